// ah_fused.hip — Compare(x OP scalar) → Filter(DropNulls) → Sum in one pass.
//
// NEW entry point (no single reference function): it computes, in one read of the
// column, exactly what the reference computes with three calls —
//   compute.CallFunction("greater", x, t)     (compute/scalar_compare.go:33,
//                                              kernels/scalar_comparisons.go:199-218;
//                                              mask validity = x validity,
//                                              compute/executor.go:237-349)
//   compute.Filter(x, mask, DropNulls)        (kernels/vector_selection.go:267-395)
//   math.Int64.Sum / math.Float64.Sum          (arrow/math/float64.go:34-47)
// i.e. Σ x[i] over { i : valid[i] ∧ x[i] OP t } and the survivor count.  Neither the
// mask nor the filtered column is materialised: 8 (+1/8) algorithmic bytes per row
// instead of 16.25 + 16·s for the unfused chain.
//
// On the streaming-reduction layer (ah_reduce.h, DESIGN.md §3 "Streaming reductions"): double-double
// accumulation for f64, wrapping uint64 for i64, one {sum, count} part per workgroup.
#include "ah_common.h"
#include "ah_ddsum.h"
#include "ah_reduce.h"

namespace {

constexpr int kBlock = kReduceBlock;
constexpr int kUnroll = kReduceUnroll;

template <typename T>
using Vec2 = T __attribute__((ext_vector_type(2)));

template <typename T, int OP>
__device__ __forceinline__ bool pred(T a, T t) {
  if (OP == AH_CMP_EQ) return a == t;
  if (OP == AH_CMP_NE) return a != t;
  if (OP == AH_CMP_GT) return a > t;
  return a >= t;
}

// the parts of the layer: one accumulator per lane
template <typename T> struct Acc;
template <> struct Acc<double> {
  ah_ddx a; unsigned long long n;   // ah_ddsum.h: the sum follows the extended reals, like ah_sum_float64
  static constexpr bool kClassed = true;
  __device__ __forceinline__ void init() { ah_ddx_init(a); n = 0; }
  __device__ __forceinline__ void add(double x) { ah_ddx_add(a, x); }
  // a row taken for an ordinary one; → its high word, sign cleared (the caller remembers the largest)
  __device__ __forceinline__ unsigned add_small(double x) { ah_dd_add(a.s, a.e, x); return ah_dd_hi_abs(x); }
  __device__ __forceinline__ void merge(const Acc& p) { ah_ddx_merge(a, p.a); n += p.n; }
};
template <> struct Acc<int64_t> {
  unsigned long long s, n;
  static constexpr bool kClassed = false;
  __device__ __forceinline__ void init() { s = 0; n = 0; }
  __device__ __forceinline__ void add(int64_t x) { s += (unsigned long long)x; }
  __device__ __forceinline__ unsigned add_small(int64_t x) { add(x); return 0; }
  __device__ __forceinline__ void merge(const Acc& p) { s += p.s; n += p.n; }
};

// body = 16-byte aligned region of nvec 2-element vectors starting at row `row0`; rows before and after it — block 0, lane 0.
// Float64: the classed rule of the layer over the KEPT rows.
template <typename T, int OP, bool HAS_VALID, bool NT>
__global__ __launch_bounds__(kBlock) void fused_kernel(const T* __restrict__ x, int64_t n, int64_t row0, int64_t nvec,
                                                        const uint8_t* __restrict__ valid, int64_t off, T thr,
                                                        Acc<T>* __restrict__ partials) {
  Acc<T> a;
  a.init();
  // vector j's two validity bits: bit 0 for .x, bit 1 for .y
  auto vbits = [&](int64_t j) -> unsigned {
    if (!HAS_VALID) return 3;
    const int64_t bit = off + row0 + 2 * j;
    return (unsigned)((valid[bit >> 3] >> (bit & 7)) & 1) | ((unsigned)((valid[(bit + 1) >> 3] >> ((bit + 1) & 7)) & 1) << 1);
  };
  ah_reduce_walk_classed<Vec2<T>, NT, Acc<T>::kClassed>(
      (const Vec2<T>*)(x + row0), nvec,
      [&](int64_t j, const Vec2<T>& v) {
        const unsigned vb = vbits(j);
        unsigned top = 0, k = 0;
        if ((vb & 1) && pred<T, OP>(v.x, thr)) { top = a.add_small(v.x); k++; }
        if ((vb & 2) && pred<T, OP>(v.y, thr)) { top = max(top, a.add_small(v.y)); k++; }
        a.n += k;
        return top;
      },
      [&](int64_t j, const Vec2<T>& v) {
        const unsigned vb = vbits(j);
        unsigned k = 0;
        if ((vb & 1) && pred<T, OP>(v.x, thr)) { a.add(v.x); k++; }
        if ((vb & 2) && pred<T, OP>(v.y, thr)) { a.add(v.y); k++; }
        a.n += k;
      },
      [&] { a.init(); });
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    auto row = [&](int64_t i) {
      if ((!HAS_VALID || ah_bit(valid, off + i)) && pred<T, OP>(x[i], thr)) { a.add(x[i]); a.n++; }
    };
    for (int64_t i = 0; i < row0; i++) row(i);
    for (int64_t i = row0 + 2 * nvec; i < n; i++) row(i);
  }
  a = ah_block_reduce<kBlock>(a);
  if (threadIdx.x == 0) partials[blockIdx.x] = a;
}

// the finish: sum, count, and (Float64 only, optional) the un-rounded accumulator for a caller that merges several of them
// (ah_comm.hip) and rounds once
template <typename T>
struct EmitFused {
  T* out_sum;
  int64_t* out_count;
  double* out_parts;
  __device__ __forceinline__ void operator()(const Acc<T>& r) const {
    if constexpr (__is_floating_point(T)) {
      *out_sum = ah_ddx_result(r.a);
      if (out_parts) { out_parts[0] = r.a.s; out_parts[1] = r.a.e; out_parts[2] = r.a.bs; out_parts[3] = r.a.be; }
    } else {
      *out_sum = (T)r.s;
    }
    *out_count = (int64_t)r.n;
  }
};

// the launch that reads the column: cmpop is one of the four (fused_dev checked)
template <typename T>
void fused_launch(ah_ctx* c, int cmpop, unsigned grid, const T* x, int64_t n, int64_t row0, int64_t nvec, const uint8_t* valid, int64_t off,
                  T thr, Acc<T>* partials) {
#define AH_FUSED(OPC)                                                                                                   \
  if (valid) {                                                                                                          \
    if (c->tune_nt) fused_kernel<T, OPC, true, true><<<grid, kBlock, 0, c->stream>>>(x, n, row0, nvec, valid, off, thr, partials);   \
    else fused_kernel<T, OPC, true, false><<<grid, kBlock, 0, c->stream>>>(x, n, row0, nvec, valid, off, thr, partials);             \
  } else {                                                                                                              \
    if (c->tune_nt) fused_kernel<T, OPC, false, true><<<grid, kBlock, 0, c->stream>>>(x, n, row0, nvec, valid, off, thr, partials);  \
    else fused_kernel<T, OPC, false, false><<<grid, kBlock, 0, c->stream>>>(x, n, row0, nvec, valid, off, thr, partials);            \
  }
  switch (cmpop) {
    case AH_CMP_EQ: AH_FUSED(AH_CMP_EQ) break;
    case AH_CMP_NE: AH_FUSED(AH_CMP_NE) break;
    case AH_CMP_GT: AH_FUSED(AH_CMP_GT) break;
    default: AH_FUSED(AH_CMP_GE) break;
  }
#undef AH_FUSED
}

template <typename T>
int fused_dev(ah_ctx* c, int cmpop, const T* x, const uint8_t* valid, int64_t off, int64_t n, T thr, T* out_sum_dev,
              int64_t* out_count_dev, double* out_parts_dev = nullptr) {
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "cmp_filter_sum: negative length/offset");
  if (n == 0) {
    AH_HIP(c, hipMemsetAsync(out_sum_dev, 0, sizeof(T), c->stream));
    AH_HIP(c, hipMemsetAsync(out_count_dev, 0, sizeof(int64_t), c->stream));
    if (out_parts_dev) AH_HIP(c, hipMemsetAsync(out_parts_dev, 0, 4 * sizeof(double), c->stream));
    return AH_OK;
  }
  if (!x) return ah_fail(c, AH_EINVALID, "cmp_filter_sum: null values");
  if ((uintptr_t)x & 7) return ah_fail(c, AH_EINVALID, "cmp_filter_sum: buffer not element-aligned");
  if (cmpop != AH_CMP_EQ && cmpop != AH_CMP_NE && cmpop != AH_CMP_GT && cmpop != AH_CMP_GE) return ah_fail(c, AH_EINVALID, "cmp_filter_sum: bad op %d", cmpop);
  const ah_split sp = ah_reduce_split(x, n);
  // validity is read with byte loads: more waves in flight pay for the extra latency (0.17 ms at
  // 8/CU vs 0.29 ms at 2/CU with 10 % nulls); without validity the reduction likes few partials
  return ah_reduce_two_launch<Acc<T>>(
      c, ah_ceil_div(sp.nvec > 0 ? sp.nvec : 1, (int64_t)kBlock * kUnroll), /*default_bpc=*/valid ? 8 : 2,
      [&](unsigned grid, Acc<T>* partials) { fused_launch<T>(c, cmpop, grid, x, n, sp.head, sp.nvec, valid, off, thr, partials); },
      EmitFused<T>{out_sum_dev, out_count_dev, out_parts_dev});
}

template <typename T>
int fused_host(ah_ctx* c, int cmpop, const T* x, const uint8_t* valid, int64_t off, int64_t n, T thr, T* out_sum_host,
               int64_t* out_count_host) {
  T* dsum = (T*)&c->dscalars[kDsFusedSum];
  int64_t* dcnt = (int64_t*)&c->dscalars[kDsFusedCount];
  int rc = fused_dev<T>(c, cmpop, x, valid, off, n, thr, dsum, dcnt);
  if (rc != AH_OK) return rc;
  { int mrc = ah_mailbox_read(c, (const unsigned long long*)dsum, 2, (unsigned long long*)c->pinned); if (mrc != AH_OK) return mrc; }
  if (out_sum_host) memcpy(out_sum_host, (const void*)&c->pinned[0], sizeof(T));
  if (out_count_host) memcpy(out_count_host, (const void*)&c->pinned[1], sizeof(int64_t));
  return AH_OK;
}

}  // namespace

AH_EXPORT int ah_cmp_filter_sum_i64(ah_ctx* c, int cmpop, const int64_t* x, const uint8_t* valid, int64_t off, int64_t n,
                                    int64_t threshold, int64_t* out_sum_host, int64_t* out_count_host) {
  AH_ENTER(c);
  return fused_host<int64_t>(c, cmpop, x, valid, off, n, threshold, out_sum_host, out_count_host);
}
AH_EXPORT int ah_cmp_filter_sum_f64(ah_ctx* c, int cmpop, const double* x, const uint8_t* valid, int64_t off, int64_t n,
                                    double threshold, double* out_sum_host, int64_t* out_count_host) {
  AH_ENTER(c);
  return fused_host<double>(c, cmpop, x, valid, off, n, threshold, out_sum_host, out_count_host);
}
AH_EXPORT int ah_cmp_filter_sum_i64_dev(ah_ctx* c, int cmpop, const int64_t* x, const uint8_t* valid, int64_t off,
                                        int64_t n, int64_t threshold, int64_t* out_sum_count_dev) {
  AH_ENTER(c);
  if (!out_sum_count_dev) return ah_fail(c, AH_EINVALID, "cmp_filter_sum: null output");
  return fused_dev<int64_t>(c, cmpop, x, valid, off, n, threshold, out_sum_count_dev, out_sum_count_dev + 1);
}
AH_EXPORT int ah_cmp_filter_sum_f64_dev(ah_ctx* c, int cmpop, const double* x, const uint8_t* valid, int64_t off,
                                        int64_t n, double threshold, double* out_sum_dev, int64_t* out_count_dev) {
  AH_ENTER(c);
  if (!out_sum_dev || !out_count_dev) return ah_fail(c, AH_EINVALID, "cmp_filter_sum: null output");
  return fused_dev<double>(c, cmpop, x, valid, off, n, threshold, out_sum_dev, out_count_dev);
}
// internal (ah_comm.hip): the sum, the count and the un-rounded four-word accumulator {s, e, bs, be} of this rank's rows
int ah_fused_f64_parts_dev(ah_ctx* c, int cmpop, const double* x, const uint8_t* valid, int64_t off, int64_t n, double threshold,
                           double* out_sum_dev, int64_t* out_count_dev, double* out_parts_dev) {
  return fused_dev<double>(c, cmpop, x, valid, off, n, threshold, out_sum_dev, out_count_dev, out_parts_dev);
}
