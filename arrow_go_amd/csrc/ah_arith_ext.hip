// ah_arith_ext.hip — the part of the arithmetic registry that knows validity or can fail: checked add / subtract / multiply,
// divide, abs / negate with overflow check, bit-wise and / or / xor / not, shifts, power, sqrt, floor / ceil / trunc, round.
//
// Reference (arrow/compute/internal/kernels):
//   add, subtract              base_arithmetic.go:249-286: the carry test, through ScalarBinaryNotNull (helpers.go:284-380)
//   multiply                   :84-106 mulWithOverflow in EVERY slot (ScalarBinary, helpers.go:193-236), null payloads included;
//                              floats under the three checked names take the unchecked kernels (base_arithmetic_amd64.go:109-117)
//   divide, divide_unchecked   base_arithmetic.go:154-160, 287-294 (integers: BOTH names refuse a zero divisor in
//                              a valid slot, "divide by zero"; Go's truncated quotient, MinInt / −1 wraps);
//                              :386-396 (floats: unchecked = IEEE a / b, checked refuses b == 0)
//                              — all through ScalarBinaryNotNull (helpers.go:284-380): null slots hold 0
//   abs, negate                :295-340 (signed integers: MinInt → "overflow", tested in EVERY slot — ScalarUnary
//                              walks the value buffer, helpers.go:56-90 — unsigned abs is a copy), floats :398-411
//   bit_wise_and / or / xor    scalar_arithmetic.go:170-245: bitmap ops over the raw value buffers, every slot
//   bit_wise_not               :253-268 ScalarUnaryNotNull: null slots hold 0
//   shift_left / shift_right   :293-378: a shift count outside [0, bits − 2] (signed) / [0, bits − 1] (unsigned)
//                              returns the left operand, and is "shift amount must be >= 0 and less than precision
//                              of type" for the checked names; ScalarBinaryNotNull
//   floor, ceil, trunc         rounding.go:180-187, 748-775: math.Floor / Ceil / Trunc in every slot (ScalarUnary), floats
//   sqrt, sqrt_unchecked       base_arithmetic.go:412-426: unchecked in every slot (ScalarUnary), checked NotNull
//                              with "square root of negative number"
// None of these has an assembly leaf in the reference (base_arithmetic_amd64.go:67-105: "no SIMD for POWER or
// SQRT", NotNull ops stay in Go), so the C signature below is derived from the Go closures.
//
// One kernel shape for all of them: 16 bytes per lane per operand, validity as V bits per lane, one flag word
// of error bits, 16-byte stores.  HBM-bound like ah_arith.hip except 64-bit integer division (≈ 100 VALU
// instructions per element).  What an element computes, and which ops skip null slots: ah_elementwise.h.
#include "ah_common.h"
#include "ah_elementwise.h"

namespace {

constexpr int kBlock = 256;

// SHAPE: 0 = l[i] ∘ r[i], 1 = l[i] ∘ scalar (and all unary ops), 2 = scalar ∘ r[i]
template <typename ST, int X, int SHAPE>
__global__ __launch_bounds__(kBlock) void ext_kernel(const ST* __restrict__ l, const uint8_t* __restrict__ lv, int64_t loff,
                                                      const ST* __restrict__ r, const uint8_t* __restrict__ rv, int64_t roff,
                                                      ST scalar, ST* __restrict__ out, int64_t len, unsigned* __restrict__ flag, int aligned) {
  constexpr int V = 16 / sizeof(ST);
  using VT = ah_vec16<ST>;
  unsigned err = 0;
  const int64_t nvec = len / V;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nvec; i += stride) {
    VT a, b, o;
    if (SHAPE != 2) a = ah_load16<ST>(l, i, aligned);
    if (SHAPE != 1) b = ah_load16<ST>(r, i, aligned);
    unsigned vbits = (1u << V) - 1;
    if (NotNull(X)) {
      if (SHAPE != 2 && lv) vbits &= (unsigned)ah_load_bits64(lv, loff + i * V, V);
      if (SHAPE != 1 && rv) vbits &= (unsigned)ah_load_bits64(rv, roff + i * V, V);
    }
#pragma unroll
    for (int e = 0; e < V; e++) {
      if constexpr (LiveSlotsOnly(X)) {
        ST v = (ST)0;
        if ((vbits >> e) & 1) v = apply<ST, X>(SHAPE == 2 ? scalar : a.v[e], SHAPE == 1 ? scalar : b.v[e], err);
        o.v[e] = v;
      } else {
        unsigned e1 = 0;
        const ST v = apply<ST, X>(SHAPE == 2 ? scalar : a.v[e], SHAPE == 1 ? scalar : b.v[e], e1);
        const bool valid = (vbits >> e) & 1;
        o.v[e] = valid ? v : (ST)0;   // helpers.go:303-306: null slots hold the zero value
        if (valid) err |= e1;
      }
    }
    ah_store16<ST>(out, i, o, aligned);
  }
  if (blockIdx.x == 0) {  // < V trailing elements
    const int64_t j = nvec * V + threadIdx.x;
    if (j < len) {
      const bool valid = !NotNull(X) || ((SHAPE == 2 || ah_bit(lv, loff + j)) && (SHAPE == 1 || ah_bit(rv, roff + j)));
      unsigned e1 = 0;
      const ST v = apply<ST, X>(SHAPE == 2 ? scalar : l[j], SHAPE == 1 ? scalar : r[j], e1);
      out[j] = valid ? v : (ST)0;
      if (valid) err |= e1;
    }
  }
  report_errors(err, flag);
}

template <typename ST, int X>
int launch(ah_ctx* c, int shape, const void* l, const uint8_t* lv, int64_t loff, const void* r, const uint8_t* rv, int64_t roff, void* out,
           int64_t len, unsigned* flag) {
  ST scalar = 0;
  if (!Unary(X)) {
    if (shape == AH_SHAPE_AS) memcpy(&scalar, r, sizeof(ST));
    if (shape == AH_SHAPE_SA) memcpy(&scalar, l, sizeof(ST));
  }
  // exact grid, one vector per lane: same finding as ah_arith.hip (no grid-stride tail, maximum loads in flight)
  const unsigned grid = ah_stream_grid(c, ah_ceil_div(len / (16 / (int64_t)sizeof(ST)) + 1, kBlock), /*default_bpc=*/0);
  const ST* pl = (const ST*)l; const ST* pr = (const ST*)r; ST* po = (ST*)out;
  const bool arr_l = !(shape == AH_SHAPE_SA && !Unary(X)), arr_r = !Unary(X) && shape != AH_SHAPE_AS;
  const int aligned = c->tune_nt && ((((uintptr_t)out) | (arr_l ? (uintptr_t)l : 0) | (arr_r ? (uintptr_t)r : 0)) & 15) == 0;
  if (Unary(X) || shape == AH_SHAPE_AS) ext_kernel<ST, X, 1><<<grid, kBlock, 0, c->stream>>>(pl, lv, loff, nullptr, nullptr, 0, scalar, po, len, flag, aligned);
  else if (shape == AH_SHAPE_AA) ext_kernel<ST, X, 0><<<grid, kBlock, 0, c->stream>>>(pl, lv, loff, pr, rv, roff, scalar, po, len, flag, aligned);
  else ext_kernel<ST, X, 2><<<grid, kBlock, 0, c->stream>>>(nullptr, nullptr, 0, pr, rv, roff, scalar, po, len, flag, aligned);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

#define AH_X(X) return launch<ST, X>(c, shape, l, lv, loff, r, rv, roff, out, len, flag)

template <typename ST>
int dispatch_int(ah_ctx* c, int op, int shape, const void* l, const uint8_t* lv, int64_t loff, const void* r, const uint8_t* rv, int64_t roff,
                 void* out, int64_t len, unsigned* flag) {
  switch (op) {
    case AH_OP_DIV: AH_X(X_DIV);
    case AH_OP_DIV_CHECKED: AH_X(X_DIV_CHECKED);
    case AH_OP_SHIFT_LEFT: AH_X(X_SHL);
    case AH_OP_SHIFT_LEFT_CHECKED: AH_X(X_SHL_CHECKED);
    case AH_OP_SHIFT_RIGHT: AH_X(X_SHR);
    case AH_OP_SHIFT_RIGHT_CHECKED: AH_X(X_SHR_CHECKED);
    case AH_OP_POWER: AH_X(X_POW);
    case AH_OP_POWER_CHECKED: AH_X(X_POW_CHECKED);
    case AH_OP_BIT_NOT: AH_X(X_BIT_NOT);
    case AH_OP_BIT_AND: AH_X(X_BIT_AND);
    case AH_OP_BIT_OR: AH_X(X_BIT_OR);
    case AH_OP_BIT_XOR: AH_X(X_BIT_XOR);
    case AH_OP_ABS_CHECKED: AH_X(X_ABS_CHECKED);
    case AH_OP_NEGATE_CHECKED:
      if ((ST)-1 > (ST)0) break;  // GetArithmeticUnarySignedKernels: no unsigned negate
      AH_X(X_NEG_CHECKED);
  }
  return ah_fail(c, AH_ENOTIMPL, "arithmetic: op %d is not defined for this integer type", op);
}

// the checked names of ah_arith.hip's three ops, integers only
template <typename ST>
int dispatch_checked(ah_ctx* c, int op, int shape, const void* l, const uint8_t* lv, int64_t loff, const void* r, const uint8_t* rv, int64_t roff,
                     void* out, int64_t len, unsigned* flag) {
  switch (op) {
    case AH_OP_ADD_CHECKED: AH_X(X_ADD_CHECKED);
    case AH_OP_SUB_CHECKED: AH_X(X_SUB_CHECKED);
    case AH_OP_MUL_CHECKED: AH_X(X_MUL_CHECKED);
  }
  return ah_fail(c, AH_ENOTIMPL, "arithmetic_checked: unsupported op %d", op);
}

template <typename ST>
int dispatch_float(ah_ctx* c, int op, int shape, const void* l, const uint8_t* lv, int64_t loff, const void* r, const uint8_t* rv, int64_t roff,
                   void* out, int64_t len, unsigned* flag) {
  switch (op) {
    case AH_OP_DIV: AH_X(X_DIV);
    case AH_OP_DIV_CHECKED: AH_X(X_DIV_CHECKED);
    case AH_OP_ABS_CHECKED: AH_X(X_ABS_CHECKED);
    case AH_OP_NEGATE_CHECKED: AH_X(X_NEG_CHECKED);
    case AH_OP_POWER: case AH_OP_POWER_CHECKED: AH_X(X_POW);
    case AH_OP_SQRT: AH_X(X_SQRT);
    case AH_OP_SQRT_CHECKED: AH_X(X_SQRT_CHECKED);
    case AH_OP_FLOOR: AH_X(X_FLOOR);
    case AH_OP_CEIL: AH_X(X_CEIL);
    case AH_OP_TRUNC: AH_X(X_TRUNC);
  }
  return ah_fail(c, AH_ENOTIMPL, "arithmetic: op %d is not defined for floating point", op);
}
#undef AH_X

// ---- round / round_to_multiple (kernels/rounding.go:321-370, 562-598) --------------------------------------------
// MODE: RoundMode (rounding.go:40-59).  MULTIPLE: round_to_multiple (scale = the multiple: divide, round, multiply);
// otherwise scale = 10^|ndigits| (multiply first when ndigits ≥ 0, divide first when negative).  Arithmetic in T, the
// rounding primitives in double — as the Go code has it.  Inf / NaN and values that are integral after scaling pass
// through; a non-finite result in a valid slot is "overflow".  ScalarUnaryNotNull: null slots hold 0.
template <typename T, bool MULTIPLE>
__global__ __launch_bounds__(kBlock) void round_kernel(const T* __restrict__ in, const uint8_t* __restrict__ valid, int64_t off, int64_t n,
                                                        T scale, int ndigits_sign, int mode, T* __restrict__ out, unsigned* __restrict__ flag) {
  unsigned err = 0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const T arg = in[i];
    T res = arg;
    if (!ah_bit(valid, off + i)) {
      res = (T)0;
    } else if (!(__builtin_isinf((double)arg) || __builtin_isnan((double)arg))) {
      T rv = (MULTIPLE || ndigits_sign < 0) ? arg / scale : arg * scale;
      const T frac = rv - (T)__builtin_floor((double)rv);
      if (frac != (T)0) {
        if (mode >= 4 && frac != (T)0.5) rv = (T)__builtin_round((double)rv);  // math.Round: half away from zero (not a tie here)
        else rv = round_impl<T>(rv, mode);
        if (MULTIPLE) rv *= scale;
        else if (ndigits_sign > 0) rv /= scale;
        else rv *= scale;
        if (__builtin_isinf((double)rv) || __builtin_isnan((double)rv)) err |= ERR_OVERFLOW;
        else res = rv;
      }
    }
    out[i] = res;
  }
  report_errors(err, flag);
}

// the flag word around a launch: cleared, `launch(flag)`, and — where the op can fail — read back and turned into the error
template <class F>
int run_flagged(ah_ctx* c, bool can_fail, F&& launch) {
  unsigned* flag = (unsigned*)c->dscalars;
  unsigned bits = 0;
  int rc = ah_flag_clear(c, flag);
  if (rc == AH_OK) rc = launch(flag);
  if (rc == AH_OK && can_fail) rc = ah_flag_read(c, flag, &bits);
  return rc == AH_OK ? ah_error_of_flag(c, bits) : rc;
}

bool is_unary_op(int op) {
  return op == AH_OP_BIT_NOT || op == AH_OP_ABS_CHECKED || op == AH_OP_NEGATE_CHECKED || op == AH_OP_SQRT || op == AH_OP_SQRT_CHECKED ||
         op == AH_OP_FLOOR || op == AH_OP_CEIL || op == AH_OP_TRUNC;
}

}  // namespace

int ah_error_of_flag(ah_ctx* c, unsigned bits) {   // first match in this order
  static const struct { unsigned bit; int code; const char* text; } kErrors[] = {
      {ERR_OVERFLOW, AH_EOVERFLOW, "overflow"},
      {ERR_DIV_ZERO, AH_EINVALID, "divide by zero"},
      {ERR_SHIFT, AH_EINVALID, "shift amount must be >= 0 and less than precision of type"},
      {ERR_NEG_SQRT, AH_EINVALID, "square root of negative number"},
      {ERR_NEG_POWER, AH_EINVALID, "integers to negative integer powers are not allowed"}};
  for (const auto& e : kErrors)
    if (bits & e.bit) return ah_fail(c, e.code, "%s", e.text);
  return AH_OK;
}

AH_EXPORT int ah_arithmetic_ext(ah_ctx* c, int type, int op, int shape, const void* l, const uint8_t* lvalid, int64_t loff, const void* r,
                                const uint8_t* rvalid, int64_t roff, int scalar_valid, void* out, int64_t len) {
  AH_ENTER(c);
  if (len < 0 || loff < 0 || roff < 0) return ah_fail(c, AH_EINVALID, "arithmetic: negative length/offset");
  if (len == 0) return AH_OK;
  const bool unary = is_unary_op(op);
  if (unary) shape = AH_SHAPE_AS;
  if (shape < AH_SHAPE_AA || shape > AH_SHAPE_SA) return ah_fail(c, AH_EINVALID, "arithmetic: bad shape %d", shape);
  const int w = ah_type_width(type);
  if (!w) return ah_fail(c, AH_ENOTIMPL, "arithmetic: unsupported type id %d", type);
  if (!out || (shape != AH_SHAPE_SA && !l) || (!unary && !r) || (shape == AH_SHAPE_SA && !l)) return ah_fail(c, AH_EINVALID, "arithmetic: null buffer");
  const void* arr0 = shape == AH_SHAPE_SA ? r : l;
  if ((((uintptr_t)arr0 | (uintptr_t)out | (shape == AH_SHAPE_AA ? (uintptr_t)r : 0)) & (uintptr_t)(w - 1)) != 0)
    return ah_fail(c, AH_EINVALID, "arithmetic: buffer not element-aligned");
  const bool every_slot = op == AH_OP_BIT_AND || op == AH_OP_BIT_OR || op == AH_OP_BIT_XOR || op == AH_OP_ABS_CHECKED || op == AH_OP_NEGATE_CHECKED ||
                          op == AH_OP_SQRT || op == AH_OP_FLOOR || op == AH_OP_CEIL || op == AH_OP_TRUNC || op == AH_OP_POWER ||
                          (op == AH_OP_POWER_CHECKED && (type == AH_FLOAT32 || type == AH_FLOAT64));
  if (!every_slot && !unary && shape != AH_SHAPE_AA && !scalar_valid) {
    // null scalar: the output stays as allocated = zero (helpers.go:312-314, 341-343)
    AH_HIP(c, hipMemsetAsync(out, 0, (size_t)len * w, c->stream));
    return AH_OK;
  }
  const bool cannot_fail = (op == AH_OP_DIV && (type == AH_FLOAT32 || type == AH_FLOAT64)) || op == AH_OP_BIT_AND || op == AH_OP_BIT_OR ||
                           op == AH_OP_BIT_XOR || op == AH_OP_BIT_NOT || op == AH_OP_SQRT || op == AH_OP_SHIFT_LEFT || op == AH_OP_SHIFT_RIGHT ||
                           op == AH_OP_FLOOR || op == AH_OP_CEIL || op == AH_OP_TRUNC;   // no readback
  return run_flagged(c, !cannot_fail, [&](unsigned* flag) {
    int rc = AH_OK;
    const bool known = with_numeric_type(type, [&](auto t) {
      using T = typename decltype(t)::type;
      if constexpr (__is_floating_point(T)) rc = dispatch_float<T>(c, op, shape, l, lvalid, loff, r, rvalid, roff, out, len, flag);
      else rc = dispatch_int<T>(c, op, shape, l, lvalid, loff, r, rvalid, roff, out, len, flag);
    });
    return known ? rc : ah_fail(c, AH_ENOTIMPL, "arithmetic: unsupported type id %d", type);
  });
}

AH_EXPORT int ah_arithmetic_checked(ah_ctx* c, int type, int8_t op, int shape,
                                    const void* l, const uint8_t* lvalid, int64_t loff,
                                    const void* r, const uint8_t* rvalid, int64_t roff,
                                    int scalar_valid, void* out, int64_t len) {
  AH_ENTER(c);
  if (len < 0) return ah_fail(c, AH_EINVALID, "arithmetic_checked: negative length");
  if (len == 0) return AH_OK;
  if (shape < AH_SHAPE_AA || shape > AH_SHAPE_SA) return ah_fail(c, AH_EINVALID, "arithmetic_checked: bad shape %d", shape);
  // floats: checked == unchecked SIMD kernels (base_arithmetic_amd64.go:109-117)
  if (type == AH_FLOAT32 || type == AH_FLOAT64) return ah_arith_binary(c, type, op, shape, l, r, out, len);
  if (op != AH_OP_ADD_CHECKED && op != AH_OP_SUB_CHECKED && op != AH_OP_MUL_CHECKED)
    return ah_fail(c, AH_ENOTIMPL, "arithmetic_checked: unsupported op %d", op);
  int w = ah_type_width(type);
  if (!w) return ah_fail(c, AH_ENOTIMPL, "arithmetic_checked: unsupported type id %d", type);
  if (op != AH_OP_MUL_CHECKED && shape != AH_SHAPE_AA && !scalar_valid) {
    // null scalar: output stays as allocated = zero (helpers.go:312-314,341-343)
    AH_HIP(c, hipMemsetAsync(out, 0, (size_t)len * w, c->stream));
    return AH_OK;
  }
  return run_flagged(c, true, [&](unsigned* flag) {
    int rc = AH_OK;
    const bool known = with_numeric_type(type, [&](auto t) {
      using T = typename decltype(t)::type;
      if constexpr (!__is_floating_point(T)) rc = dispatch_checked<T>(c, op, shape, l, lvalid, loff, r, rvalid, roff, out, len, flag);
    });
    return known ? rc : ah_fail(c, AH_ENOTIMPL, "arithmetic_checked: unsupported type id %d", type);
  });
}

AH_EXPORT int ah_round(ah_ctx* c, int type, const void* values, const uint8_t* valid, int64_t off, int64_t n, int64_t ndigits, int mode,
                       const void* multiple_host, double pow10, void* out) {
  AH_ENTER(c);
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "round: negative length/offset");
  if (mode < 0 || mode > 9) return ah_fail(c, AH_EINVALID, "round: invalid rounding mode %d", mode);
  if (type != AH_FLOAT32 && type != AH_FLOAT64) return ah_fail(c, AH_ENOTIMPL, "round: unsupported type id %d", type);
  if (n == 0) return AH_OK;
  if (!values || !out) return ah_fail(c, AH_EINVALID, "round: null buffer");
  const unsigned grid = ah_stream_grid(c, ah_ceil_div(n, kBlock), /*default_bpc=*/8);
  const int sgn = ndigits > 0 ? 1 : (ndigits < 0 ? -1 : 0);
  return run_flagged(c, true, [&](unsigned* flag) {
    if (type == AH_FLOAT32) {
      float scale = (float)pow10;
      if (multiple_host) { memcpy(&scale, multiple_host, 4); round_kernel<float, true><<<grid, kBlock, 0, c->stream>>>((const float*)values, valid, off, n, scale, 0, mode, (float*)out, flag); }
      else round_kernel<float, false><<<grid, kBlock, 0, c->stream>>>((const float*)values, valid, off, n, scale, sgn, mode, (float*)out, flag);
    } else {
      double scale = pow10;
      if (multiple_host) { memcpy(&scale, multiple_host, 8); round_kernel<double, true><<<grid, kBlock, 0, c->stream>>>((const double*)values, valid, off, n, scale, 0, mode, (double*)out, flag); }
      else round_kernel<double, false><<<grid, kBlock, 0, c->stream>>>((const double*)values, valid, off, n, scale, sgn, mode, (double*)out, flag);
    }
    AH_LAUNCH_CHECK(c);
    return (int)AH_OK;
  });
}
