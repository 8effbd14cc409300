// ah_arith.hip — element-wise ADD / SUB / MUL (array∘array, array∘scalar,
// scalar∘array) and ABS / NEGATE / SIGN.  What an element computes: ah_elementwise.h; the
// checked integer variants: ah_arith_ext.hip.
//
// Replaces: _arithmetic_binary_avx2, _arithmetic_arr_scalar_avx2,
//   _arithmetic_scalar_arr_avx2, _arithmetic_unary_same_types_avx2
//   (kernels/base_arithmetic_avx2_amd64.go:27-60; C truth
//   kernels/_lib/base_arithmetic.cc:52-273,441-483; Go loop
//   kernels/base_arithmetic.go:110-134), reached from compute.Add/Subtract/Multiply
//   through ScalarBinary (kernels/helpers.go:193-236).
//
// Roofline: HBM, 3·w bytes per row (2·w for a scalar operand), no reuse.  One
// 16-byte vector per lane per operand (global_load_dwordx4 / global_store_dwordx4,
// nontemporal), kUnroll vectors in flight per lane, grid-stride.  Integer ops are
// done in the unsigned type of the same width (two's-complement wraparound, as the
// C source does for MUL :107-124 and the SIMD lanes do for ADD/SUB).
#include <type_traits>
#include "ah_common.h"
#include "ah_elementwise.h"

namespace {

constexpr int kBlock = 256;
constexpr int kUnroll = 4;

template <typename T>
using Vec16 = T __attribute__((ext_vector_type(16 / sizeof(T))));

template <typename V, bool NT>
__device__ __forceinline__ V vload(const V* p) {
  if (NT) return __builtin_nontemporal_load(p);
  return *p;
}
template <typename V, bool NT>
__device__ __forceinline__ void vstore(V* p, V v) {
  if (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// SHAPE: 0 = l[i] op r[i], 1 = l[i] op s, 2 = s op r[i]   (array operand in `a`,
// for shape 0 the second array in `b`).  ALIGNED: all pointers 16-byte aligned →
// ext-vector accesses; otherwise element-aligned 16-byte structs (Arrow slices).
template <typename T, int OP, int SHAPE, bool ALIGNED, bool NT>
__global__ __launch_bounds__(kBlock) void binary_kernel(const T* __restrict__ a, const T* __restrict__ b,
                                                         T* __restrict__ out, int64_t len, T scalar, unsigned xmap) {
  constexpr int V = 16 / sizeof(T);
  using VT = typename std::conditional<ALIGNED, Vec16<T>, ah_vec16<T>>::type;
  const int64_t nvec = len / V;
  const VT* av = (const VT*)a;
  const VT* bv = (const VT*)b;
  VT* ov = (VT*)out;
  const int64_t stride = (int64_t)gridDim.x * kBlock * kUnroll;
  // xmap (measurement switch arith_xcd_map): block b runs on XCD b & 7 — give every XCD one contiguous eighth of the columns
  const unsigned bid = xmap ? (blockIdx.x & 7u) * xmap + (blockIdx.x >> 3) : blockIdx.x;
  int64_t i = (int64_t)bid * kBlock * kUnroll + threadIdx.x;
  auto compute = [&](const VT& x, const VT& y) {
    VT o;
#pragma unroll
    for (int e = 0; e < V; e++) {
      T xe, ye;
      if constexpr (ALIGNED) { xe = x[e]; ye = SHAPE == 0 ? y[e] : scalar; }
      else { xe = x.v[e]; ye = SHAPE == 0 ? y.v[e] : scalar; }
      T r = SHAPE == 2 ? apply_binary<T, OP>(ye, xe) : apply_binary<T, OP>(xe, ye);
      if constexpr (ALIGNED) o[e] = r; else o.v[e] = r;
    }
    return o;
  };
  for (; i + (int64_t)(kUnroll - 1) * kBlock < nvec; i += stride) {
    VT x[kUnroll], y[kUnroll] = {};
#pragma unroll
    for (int k = 0; k < kUnroll; k++) {
      if constexpr (ALIGNED) {
        x[k] = vload<VT, NT>(&av[i + (int64_t)k * kBlock]);
        if (SHAPE == 0) y[k] = vload<VT, NT>(&bv[i + (int64_t)k * kBlock]);
      } else {
        x[k] = NT ? ah_ld16_nt<T>((const T*)(av + (i + (int64_t)k * kBlock))) : ah_ld16<T>((const T*)(av + (i + (int64_t)k * kBlock)));
        if (SHAPE == 0) y[k] = NT ? ah_ld16_nt<T>((const T*)(bv + (i + (int64_t)k * kBlock))) : ah_ld16<T>((const T*)(bv + (i + (int64_t)k * kBlock)));
      }
    }
#pragma unroll
    for (int k = 0; k < kUnroll; k++) {
      VT o = compute(x[k], y[k]);
      if constexpr (ALIGNED) vstore<VT, NT>(&ov[i + (int64_t)k * kBlock], o);
      else if constexpr (NT) ah_st16_nt<T>((T*)(ov + (i + (int64_t)k * kBlock)), o);
      else ah_st16<T>((T*)(ov + (i + (int64_t)k * kBlock)), o);
    }
  }
#pragma unroll
  for (int k = 0; k < kUnroll; k++) {
    int64_t j = i + (int64_t)k * kBlock;
    if (j < nvec) {
      VT x = av[j], y = x;
      if (SHAPE == 0) y = bv[j];
      ov[j] = compute(x, y);
    }
  }
  // scalar tail (< V elements) — block 0
  if (blockIdx.x == 0) {
    int64_t j = nvec * V + threadIdx.x;
    if (j < len) {
      T xe = a[j], ye = SHAPE == 0 ? b[j] : scalar;
      out[j] = SHAPE == 2 ? apply_binary<T, OP>(ye, xe) : apply_binary<T, OP>(xe, ye);
    }
  }
}

template <typename ST, int OP, bool ALIGNED, bool NT>
__global__ __launch_bounds__(kBlock) void unary_kernel(const ST* __restrict__ a, ST* __restrict__ out, int64_t len) {
  constexpr int V = 16 / sizeof(ST);
  using VT = typename std::conditional<ALIGNED, Vec16<ST>, ah_vec16<ST>>::type;
  const int64_t nvec = len / V;
  const VT* av = (const VT*)a;
  VT* ov = (VT*)out;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += stride) {
    VT x, o;
    if constexpr (ALIGNED) x = vload<VT, NT>(&av[i]); else x = ah_ld16<ST>((const ST*)(av + i));
#pragma unroll
    for (int e = 0; e < V; e++) {
      if constexpr (ALIGNED) o[e] = apply_unary<ST, OP>(x[e]);
      else o.v[e] = apply_unary<ST, OP>(x.v[e]);
    }
    if constexpr (ALIGNED) vstore<VT, NT>(&ov[i], o); else ah_st16<ST>((ST*)(ov + i), o);
  }
  if (blockIdx.x == 0) {
    int64_t j = nvec * V + threadIdx.x;
    if (j < len) out[j] = apply_unary<ST, OP>(a[j]);
  }
}

template <typename T, int OP, int SHAPE>
int launch_binary(ah_ctx* c, const void* a, const void* b, void* out, int64_t len, T scalar) {
  constexpr int V = 16 / sizeof(T);
  bool aligned = (((uintptr_t)a | (uintptr_t)out | (SHAPE == 0 ? (uintptr_t)b : 0)) & 15) == 0;
  int64_t iters = ah_ceil_div(len / V + 1, (int64_t)kBlock * kUnroll);
  unsigned grid = ah_stream_grid(c, iters, /*default_bpc=*/0);
  unsigned xmap = 0;
  if (c->opt_arith_xcd_map && grid >= 64) { grid = (grid + 7u) & ~7u; xmap = grid >> 3; }
  const T* pa = (const T*)a; const T* pb = (const T*)b; T* po = (T*)out;
  if (aligned) {
    if (c->tune_nt) binary_kernel<T, OP, SHAPE, true, true><<<grid, kBlock, 0, c->stream>>>(pa, pb, po, len, scalar, xmap);
    else binary_kernel<T, OP, SHAPE, true, false><<<grid, kBlock, 0, c->stream>>>(pa, pb, po, len, scalar, xmap);
  } else {   // an element-aligned slice: the same 16-byte accesses and hints at the elements' alignment
    if (c->tune_nt) binary_kernel<T, OP, SHAPE, false, true><<<grid, kBlock, 0, c->stream>>>(pa, pb, po, len, scalar, xmap);
    else binary_kernel<T, OP, SHAPE, false, false><<<grid, kBlock, 0, c->stream>>>(pa, pb, po, len, scalar, xmap);
  }
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

template <typename T>
int dispatch_binary_op(ah_ctx* c, int op, int shape, const void* l, const void* r, void* out, int64_t len) {
  // for shapes AS/SA the scalar operand is HOST memory
  T scalar = 0;
  const void* a = l; const void* b = r;
  if (shape == AH_SHAPE_AS) { memcpy(&scalar, r, sizeof(T)); b = nullptr; }
  if (shape == AH_SHAPE_SA) { memcpy(&scalar, l, sizeof(T)); a = r; b = nullptr; }
#define AH_SHAPE_SWITCH(OPC)                                                              \
  switch (shape) {                                                                        \
    case AH_SHAPE_AA: return launch_binary<T, OPC, 0>(c, a, b, out, len, scalar);         \
    case AH_SHAPE_AS: return launch_binary<T, OPC, 1>(c, a, b, out, len, scalar);         \
    case AH_SHAPE_SA: return launch_binary<T, OPC, 2>(c, a, b, out, len, scalar);         \
  }
  switch (op) {
    case AH_OP_ADD: case AH_OP_ADD_CHECKED: AH_SHAPE_SWITCH(OP_ADD) break;
    case AH_OP_SUB: case AH_OP_SUB_CHECKED: AH_SHAPE_SWITCH(OP_SUB) break;
    case AH_OP_MUL: case AH_OP_MUL_CHECKED: AH_SHAPE_SWITCH(OP_MUL) break;
  }
#undef AH_SHAPE_SWITCH
  return ah_fail(c, AH_ENOTIMPL, "arithmetic: unsupported op %d / shape %d", op, shape);
}

template <typename ST>
int dispatch_unary(ah_ctx* c, int op, const void* in, void* out, int64_t len) {
  constexpr int V = 16 / sizeof(ST);
  bool aligned = (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
  unsigned grid = ah_stream_grid(c, ah_ceil_div(len / V + 1, kBlock), /*default_bpc=*/0);
  const ST* a = (const ST*)in; ST* o = (ST*)out;
#define AH_UNARY(OPC)                                                                          \
  if (aligned) unary_kernel<ST, OPC, true, true><<<grid, kBlock, 0, c->stream>>>(a, o, len);   \
  else unary_kernel<ST, OPC, false, false><<<grid, kBlock, 0, c->stream>>>(a, o, len);
  switch (op) {
    case AH_OP_ABS: AH_UNARY(OP_ABS) break;
    case AH_OP_NEGATE: AH_UNARY(OP_NEG) break;
    case AH_OP_SIGN: AH_UNARY(OP_SIGN) break;
    default: return ah_fail(c, AH_ENOTIMPL, "arithmetic_unary: unsupported op %d", op);
  }
#undef AH_UNARY
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

}  // namespace

int ah_arith_binary(ah_ctx* c, int type, int op, int shape, const void* l, const void* r, void* out, int64_t len) {
  if (len < 0) return ah_fail(c, AH_EINVALID, "arithmetic: negative length");
  if (len == 0) return AH_OK;
  int w = ah_type_width(type);
  if (!w) return ah_fail(c, AH_ENOTIMPL, "arithmetic: unsupported type id %d", type);
  const void* arr0 = shape == AH_SHAPE_SA ? r : l;
  if ((((uintptr_t)arr0 | (uintptr_t)out | (shape == AH_SHAPE_AA ? (uintptr_t)r : 0)) & (uintptr_t)(w - 1)) != 0)
    return ah_fail(c, AH_EINVALID, "arithmetic: buffer not element-aligned");
  int rc = AH_OK;
  if (with_numeric_carrier(type, [&](auto t) { rc = dispatch_binary_op<typename decltype(t)::type>(c, op, shape, l, r, out, len); })) return rc;
  return ah_fail(c, AH_ENOTIMPL, "arithmetic: unsupported type id %d", type);
}

AH_EXPORT int ah_arithmetic_binary(ah_ctx* c, int type, int8_t op, const void* l, const void* r, void* out, int64_t len) {
  AH_ENTER(c);
  return ah_arith_binary(c, type, op, AH_SHAPE_AA, l, r, out, len);
}
AH_EXPORT int ah_arithmetic_arr_scalar(ah_ctx* c, int type, int8_t op, const void* l, const void* r_host, void* out, int64_t len) {
  AH_ENTER(c);
  if (!r_host) return ah_fail(c, AH_EINVALID, "arithmetic_arr_scalar: null scalar");
  return ah_arith_binary(c, type, op, AH_SHAPE_AS, l, r_host, out, len);
}
AH_EXPORT int ah_arithmetic_scalar_arr(ah_ctx* c, int type, int8_t op, const void* l_host, const void* r, void* out, int64_t len) {
  AH_ENTER(c);
  if (!l_host) return ah_fail(c, AH_EINVALID, "arithmetic_scalar_arr: null scalar");
  return ah_arith_binary(c, type, op, AH_SHAPE_SA, l_host, r, out, len);
}

AH_EXPORT int ah_arithmetic_unary(ah_ctx* c, int type, int8_t op, const void* in, void* out, int64_t len) {
  AH_ENTER(c);
  if (len < 0) return ah_fail(c, AH_EINVALID, "arithmetic_unary: negative length");
  if (len == 0) return AH_OK;
  int rc = AH_OK;
  if (with_numeric_type(type, [&](auto t) { rc = dispatch_unary<typename decltype(t)::type>(c, op, in, out, len); })) return rc;
  return ah_fail(c, AH_ENOTIMPL, "arithmetic_unary: unsupported type id %d", type);
}
