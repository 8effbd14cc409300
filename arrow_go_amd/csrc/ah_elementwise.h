// ah_elementwise.h — what one element of an element-wise kernel computes, stated once: ah_arith.hip (add / subtract / multiply,
// abs / negate / sign), ah_arith_ext.hip (everything with validity or an error: checked ops, divide, shifts, bit-wise, power, sqrt,
// floor / ceil / trunc, round) and the fused expression kernel of ah_expr.hip, which reads this very text through hiprtc — so
// "fused == per-call, byte for byte" holds by construction.  For that reader the header includes nothing and takes its type
// traits from the compiler (__is_floating_point, (T)-1 < (T)0) or states them (unsigned_of: __make_unsigned is a keyword only
// until the host's standard library declares a template of that name).  Device code only: the error bits' texts are
// ah_error_of_flag (ah_arith_ext.hip).
#pragma once

namespace {

template <int W> struct UIntOfBytes;
template <> struct UIntOfBytes<1> { using type = unsigned char; };
template <> struct UIntOfBytes<2> { using type = unsigned short; };
template <> struct UIntOfBytes<4> { using type = unsigned int; };
template <> struct UIntOfBytes<8> { using type = unsigned long long; };
template <typename T> using unsigned_of = typename UIntOfBytes<sizeof(T)>::type;

enum { OP_ADD = 0, OP_SUB = 1, OP_MUL = 2, OP_ABS = 3, OP_NEG = 4, OP_SIGN = 5 };

// Integer ops are done in the unsigned type of the same width (two's-complement wraparound, as the C source does for MUL,
// kernels/_lib/base_arithmetic.cc:107-124, and the SIMD lanes do for ADD/SUB): the callers pass T = the unsigned carrier.
template <typename T, int OP>
__device__ __forceinline__ T apply_binary(T a, T b) {
  if (OP == OP_ADD) return (T)(a + b);
  if (OP == OP_SUB) return (T)(a - b);
  return (T)(a * b);
}

// unary ops need signedness: ST is the logical (possibly signed / float) type
template <typename ST, int OP>
__device__ __forceinline__ ST apply_unary(ST x) {
  if constexpr (__is_floating_point(ST)) {
    if (OP == OP_ABS) return __builtin_fabs(x);  // clears the sign bit (base_arithmetic.cc:139-146)
    if (OP == OP_NEG) return -x;
    return __builtin_isnan(x) ? x : (x == 0 ? (ST)0 : (__builtin_signbit(x) ? (ST)-1 : (ST)1));
  } else if constexpr ((ST)-1 > (ST)0) {  // unsigned
    if (OP == OP_ABS) return x;
    if (OP == OP_NEG) return (ST)(~x + 1);
    return (ST)(x > 0 ? 1 : 0);
  } else {
    using U = unsigned_of<ST>;
    if (OP == OP_ABS) {
      U m = x < 0 ? (U)~(U)0 : (U)0;
      return (ST)(((U)x + m) ^ m);
    }
    if (OP == OP_NEG) return (ST)((U)0 - (U)x);
    return (ST)(x > 0 ? 1 : (x ? -1 : 0));
  }
}

// ---- ops with validity or an error (reference: arrow/compute/internal/kernels; the table is at the top of ah_arith_ext.hip) ----
// A NotNull op writes 0 and reports nothing in a null slot (ScalarBinaryNotNull / ScalarUnaryNotNull, helpers.go:284-380); an
// every-slot op computes and reports in every slot, null payloads included (ScalarBinary / ScalarUnary, helpers.go:56-90, 193-236).
// The kernel owns that rule; apply<ST, X> is the slot's value and its error bits.
enum { ERR_OVERFLOW = 1, ERR_DIV_ZERO = 2, ERR_SHIFT = 4, ERR_NEG_SQRT = 8, ERR_NEG_POWER = 16 };
enum { X_DIV, X_DIV_CHECKED, X_SHL, X_SHL_CHECKED, X_SHR, X_SHR_CHECKED, X_POW_CHECKED, X_BIT_NOT, X_SQRT_CHECKED, X_ADD_CHECKED, X_SUB_CHECKED,  // NotNull
       X_ABS_CHECKED, X_NEG_CHECKED, X_BIT_AND, X_BIT_OR, X_BIT_XOR, X_POW, X_MUL_CHECKED, X_SQRT, X_FLOOR, X_CEIL, X_TRUNC };  // every slot

static_assert(X_ADD_CHECKED == 9, "tests/test_isa_hints.py pins ext_kernel<long, X_ADD_CHECKED, 0> by this ordinal in its mangled name");

constexpr bool NotNull(int x) { return x <= X_SUB_CHECKED; }
// the rows a kernel evaluates in live slots only, under a branch per element — as checked_kernel did: little in flight, few registers
// (Int8 add at 48 VGPRs where computing all sixteen slots and selecting takes 58); the other rows are computed and selected
constexpr bool LiveSlotsOnly(int x) { return x == X_ADD_CHECKED || x == X_SUB_CHECKED || x == X_MUL_CHECKED; }
constexpr bool Unary(int x) { return x == X_BIT_NOT || x == X_SQRT_CHECKED || x == X_ABS_CHECKED || x == X_NEG_CHECKED || x >= X_SQRT; }

template <typename ST, int X>
__device__ __forceinline__ ST apply(ST a, ST b, unsigned& err) {
  constexpr bool kFloat = __is_floating_point(ST);
  constexpr bool kSigned = !kFloat && ((ST)-1 < (ST)0);
  constexpr int bits = sizeof(ST) * 8;
  if constexpr (X == X_ADD_CHECKED || X == X_SUB_CHECKED || X == X_MUL_CHECKED) {
    if constexpr (kFloat) {  // checked == unchecked for floats (base_arithmetic_amd64.go:109-117)
      return X == X_ADD_CHECKED ? a + b : X == X_SUB_CHECKED ? a - b : a * b;
    } else if constexpr (X == X_MUL_CHECKED) {
      // mulWithOverflow (base_arithmetic.go:84-106), every slot (ScalarBinary), null payloads included
      using U = unsigned_of<ST>;
      constexpr ST tmin = kSigned ? (ST)((U)1 << (bits - 1)) : (ST)0;
      constexpr ST tmax = kSigned ? (ST)(~((U)1 << (bits - 1))) : (ST)~(U)0;
      bool o = false;
      if (a > 0) { if (b > 0) { if (a > (ST)(tmax / b)) o = true; } else { if (b < (ST)(tmin / a)) o = true; } }
      else if (b > 0) { if (a < (ST)(tmin / b)) o = true; }
      else { if (a != 0 && b < (ST)(tmax / a)) o = true; }
      err |= o ? ERR_OVERFLOW : 0;
      return o ? (ST)0 : (ST)((U)a * (U)b);
    } else {
      using U = unsigned_of<ST>;
      U ua = (U)a, ub = (U)b, o, cy;
      if (X == X_ADD_CHECKED) { o = (U)(ua + ub); cy = (U)((ua & ub) | ((ua | ub) & (U)~o)); }
      else { o = (U)(ua - ub); cy = (U)(((U)~ua & ub) | ((U) ~(ua ^ ub) & o)); }
      // `carry > 0` after an ARITHMETIC shift by bits-2 for signed T, logical shift by bits-1 for
      // unsigned T (base_arithmetic.go:250-262): signed ⇒ top carry bit clear ∧ next bit set
      bool top = (cy >> (bits - 1)) & 1, next = (cy >> (bits - 2)) & 1;
      if (kSigned ? (!top && next) : top) err |= ERR_OVERFLOW;
      return (ST)o;
    }
  } else if constexpr (X == X_DIV || X == X_DIV_CHECKED) {
    if constexpr (kFloat) {
      if (X == X_DIV_CHECKED && b == 0) { err |= ERR_DIV_ZERO; return (ST)0; }
      return a / b;
    } else {
      using U = unsigned_of<ST>;
      if (b == 0) { err |= ERR_DIV_ZERO; return (ST)0; }
      if constexpr (kSigned) { if (b == (ST)-1) return (ST)((U)0 - (U)a); }  // MinInt / −1 wraps (Go spec, "Integer overflow")
      return (ST)(a / b);
    }
  } else if constexpr (X == X_SHL || X == X_SHL_CHECKED || X == X_SHR || X == X_SHR_CHECKED) {
    using U = unsigned_of<ST>;
    constexpr ST maxshift = kSigned ? (ST)(bits - 1) : (ST)bits;  // unsigned 8-bit: bits = 8 fits
    const bool bad = kSigned ? (b < 0 || b >= maxshift) : ((unsigned long long)b >= (unsigned long long)bits);
    if (bad) { if (X == X_SHL_CHECKED || X == X_SHR_CHECKED) err |= ERR_SHIFT; return a; }
    if (X == X_SHL || X == X_SHL_CHECKED) return (ST)((U)a << (int)b);
    return (ST)(a >> (int)b);  // arithmetic for signed, logical for unsigned
  } else if constexpr (X == X_BIT_NOT) {
    return (ST)~a;
  } else if constexpr (X == X_BIT_AND) {
    return (ST)(a & b);
  } else if constexpr (X == X_BIT_OR) {
    return (ST)(a | b);
  } else if constexpr (X == X_BIT_XOR) {
    return (ST)(a ^ b);
  } else if constexpr (X == X_ABS_CHECKED || X == X_NEG_CHECKED) {
    if constexpr (kFloat) {
      return X == X_ABS_CHECKED ? (ST)__builtin_fabs(a) : -a;
    } else if constexpr (!kSigned) {
      return a;  // abs of an unsigned value; negate has no unsigned kernel
    } else {
      using U = unsigned_of<ST>;
      constexpr ST tmin = (ST)((U)1 << (bits - 1));
      if (a == tmin) { err |= ERR_OVERFLOW; return (ST)0; }
      return X == X_ABS_CHECKED ? (ST)(a < 0 ? -a : a) : (ST)-a;
    }
  } else if constexpr (X == X_POW || X == X_POW_CHECKED) {
    // power_unchecked / power (base_arithmetic.go:226-248, 342-373, 443-446)
    if constexpr (kFloat) {
      return (ST)::pow((double)a, (double)b);      // OutT(math.Pow(float64(a), float64(b))) under both names
    } else {
      if constexpr (kSigned) {
        if (b < 0) { err |= ERR_NEG_POWER; return (ST)0; }
      }
      if constexpr (X == X_POW) {  // right to left in uint64, narrowed at the end: wraps
        unsigned long long base = (unsigned long long)a, e = (unsigned long long)b, p = 1;
        while (e != 0) {
          if (e & 1) p *= base;
          base *= base;
          e >>= 1;
        }
        return (ST)p;
      } else {  // left to right with mulWithOverflow (:84-108: an overflowing product is 0 and the flag sticks)
        if (b == 0) return (ST)1;
        const unsigned long long ue = (unsigned long long)b;
        unsigned long long mask = 1ull << (63 - __builtin_clzll(ue));
        ST p = (ST)1;
        bool of = false;
        while (mask != 0) {
          ST t;
          if (__builtin_mul_overflow(p, p, &t)) { of = true; t = (ST)0; }
          p = t;
          if (ue & mask) {
            if (__builtin_mul_overflow(p, a, &t)) { of = true; t = (ST)0; }
            p = t;
          }
          mask >>= 1;
        }
        if (of) err |= ERR_OVERFLOW;
        return p;
      }
    }
  } else if constexpr (X == X_FLOOR || X == X_CEIL || X == X_TRUNC) {
    // getFloatRoundImpl (rounding.go:180-187): math.Floor / Ceil / Trunc of the value widened to float64 and narrowed
    // back — exact in the narrow type as well
    if constexpr (kFloat) {
      const double v = (double)a;
      return (ST)(X == X_FLOOR ? __builtin_floor(v) : X == X_CEIL ? __builtin_ceil(v) : __builtin_trunc(v));
    } else {
      return a;
    }
  } else {  // X_SQRT, X_SQRT_CHECKED
    if constexpr (kFloat) {
      if (X == X_SQRT_CHECKED && a < 0) { err |= ERR_NEG_SQRT; return (ST)__builtin_nan(""); }
      return sizeof(ST) == 4 ? (ST)__builtin_sqrtf((float)a) : (ST)__builtin_sqrt((double)a);
    } else {
      return a;
    }
  }
}

// the rounding primitive of round / round_to_multiple by RoundMode (rounding.go:40-59), in double as the Go code has it
template <typename T>
__device__ __forceinline__ T round_impl(T v, int mode) {
  const double d = (double)v;
  switch (mode) {
    case 0: case 4: return (T)__builtin_floor(d);                                   // RoundDown, HalfDown (tie)
    case 1: case 5: return (T)__builtin_ceil(d);                                    // RoundUp, HalfUp (tie)
    case 2: case 6: return (T)__builtin_trunc(d);                                   // TowardsZero, HalfTowardsZero (tie)
    case 3: case 7: return (T)(__builtin_signbit(d) ? __builtin_floor(d) : __builtin_ceil(d));  // AwayFromZero, HalfAwayFromZero (tie)
    case 8: return (T)__builtin_rint(d);                                            // HalfToEven: math.RoundToEven
    default: return (T)(__builtin_floor(d * 0.5) + __builtin_ceil(d * 0.5));        // HalfToOdd
  }
}

// a kernel's last statement: the error bits its lanes collected, into the flag word — one atomic per wave and bit seen, none otherwise
__device__ __forceinline__ void report_errors(unsigned err, unsigned* __restrict__ flag) {
  for (unsigned bit = 1; bit <= ERR_NEG_POWER; bit <<= 1)
    if (__any((err & bit) != 0) && (threadIdx.x & 63) == 0) atomicOr(flag, bit);
}

}  // namespace
