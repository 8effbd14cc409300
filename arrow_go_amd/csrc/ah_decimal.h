// ah_decimal.h — the limb arithmetic of Decimal128 / Decimal256 values, shared by the decimal comparisons (ah_compare_binary.hip) and
// the decimal casts (ah_cast_decimal.hip).
//
// A decimal is its unscaled integer: 2 or 4 little-endian 64-bit limbs, two's complement.  What the reference does through math/big
// (arrow/decimal128/decimal128.go:436-526, decimal256.go: IncreaseScaleBy, ReduceScaleBy, Rescale, FitsInPrecision) is done here on
// the limbs: multiplication by 10^k in steps of at most 10^19 (one 64 × 64 → 128 multiply per limb and step), truncated division by
// 10^k in the same steps with a precomputed reciprocal per step (Möller & Granlund, "Improved division by invariant integers", 2011,
// algorithm 4: no hardware or emulated division), and the remainder tests from r = x − q·10^k.  Multiplication and division work on
// the MAGNITUDE of a value; the sign is taken off before and put back after.
//
// The arithmetic compiles for the host as well (plain C++ with unsigned __int128): tests/test_decimal_host.py checks it against
// Python integers without a GPU.  The 16-byte loads and stores are device-only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AH_DEC_FN __device__ __forceinline__
#define AH_DEC_TABLE __attribute__((unused)) static __constant__
#else
#define AH_DEC_FN static inline
#define AH_DEC_TABLE __attribute__((unused)) static const
#endif

struct I256 { unsigned long long w[4]; };

AH_DEC_TABLE unsigned long long kPow10[20] = {1ull,
                                              10ull,
                                              100ull,
                                              1000ull,
                                              10000ull,
                                              100000ull,
                                              1000000ull,
                                              10000000ull,
                                              100000000ull,
                                              1000000000ull,
                                              10000000000ull,
                                              100000000000ull,
                                              1000000000000ull,
                                              10000000000000ull,
                                              100000000000000ull,
                                              1000000000000000ull,
                                              10000000000000000ull,
                                              100000000000000000ull,
                                              1000000000000000000ull,
                                              10000000000000000000ull};

#if defined(__HIPCC__)
using V2u64 = unsigned long long __attribute__((ext_vector_type(2)));
struct V2u64u { V2u64 v; } __attribute__((packed, aligned(1)));

template <int W>
__device__ __forceinline__ I256 load_dec(const uint8_t* p) {
  I256 x;
  const V2u64 lo = reinterpret_cast<const V2u64u*>(p)->v;
  x.w[0] = lo.x;
  x.w[1] = lo.y;
  if constexpr (W == 32) {
    const V2u64 hi = reinterpret_cast<const V2u64u*>(p + 16)->v;
    x.w[2] = hi.x;
    x.w[3] = hi.y;
  } else {
    x.w[2] = x.w[3] = (unsigned long long)((long long)x.w[1] >> 63);  // sign extension
  }
  return x;
}
#endif

// x · 10^k mod 2^256: exact whenever the product fits, which the promoted precision (≤ 76 digits) guarantees
AH_DEC_FN void scale_up(I256& x, int k) {
  while (k > 0) {
    const unsigned long long m = kPow10[k < 19 ? k : 19];
    k -= 19;
    unsigned long long carry = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const unsigned __int128 p = (unsigned __int128)x.w[t] * m + carry;
      x.w[t] = (unsigned long long)p;
      carry = (unsigned long long)(p >> 64);
    }
  }
}

// ---- the casts' share: N = 2 (128 bits) or 4 (256 bits) limbs -------------------------------------------------------------------
// 10^j normalised (shifted left until bit 63 is set), its reciprocal ⌊(2^128 − 1) / d⌋ − 2^64 and the shift, j = 0 … 19
AH_DEC_TABLE unsigned long long kPow10Norm[20] = {
    9223372036854775808ull,  11529215046068469760ull, 14411518807585587200ull, 18014398509481984000ull, 11258999068426240000ull,
    14073748835532800000ull, 17592186044416000000ull, 10995116277760000000ull, 13743895347200000000ull, 17179869184000000000ull,
    10737418240000000000ull, 13421772800000000000ull, 16777216000000000000ull, 10485760000000000000ull, 13107200000000000000ull,
    16384000000000000000ull, 10240000000000000000ull, 12800000000000000000ull, 16000000000000000000ull, 10000000000000000000ull};
AH_DEC_TABLE unsigned long long kPow10Recip[20] = {
    18446744073709551615ull, 11068046444225730969ull, 5165088340638674452ull,  442721857769029238ull,  11776401416656177751ull,
    5731772318583031878ull,  896069040124515179ull,   12501756908424955256ull, 6312056711998053881ull, 1360296554856532782ull,
    13244520931996183421ull, 6906267930855036413ull,  1835665529942118807ull,  14005111292133121062ull, 7514740218964586526ull,
    2322443360429758898ull,  14783955820913345206ull, 8137815841988765842ull,  2820903858849102350ull, 15581492618384294730ull};
AH_DEC_TABLE int kPow10Shift[20] = {63, 60, 57, 54, 50, 47, 44, 40, 37, 34, 30, 27, 24, 20, 17, 14, 10, 7, 4, 0};

template <int N>
AH_DEC_FN bool dec_is_negative(const unsigned long long (&w)[N]) {
  return (long long)w[N - 1] < 0;
}

// two's complement negation; the magnitude of −2^(64N−1) is itself, read as unsigned
template <int N>
AH_DEC_FN void dec_negate(unsigned long long (&w)[N]) {
  unsigned long long carry = 1;
#pragma unroll
  for (int t = 0; t < N; t++) {
    const unsigned long long v = ~w[t] + carry;
    carry = (carry && v == 0) ? 1 : 0;
    w[t] = v;
  }
}

// unsigned a < b
template <int N>
AH_DEC_FN bool dec_less(const unsigned long long (&a)[N], const unsigned long long (&b)[N]) {
  bool lt = false;
#pragma unroll
  for (int t = 0; t < N; t++) lt = a[t] < b[t] || (a[t] == b[t] && lt);
  return lt;
}

// FitsInPrecision (decimal128.go:522-526) on a magnitude: |v| < 10^p, the bound's limbs given
template <int N>
AH_DEC_FN bool dec_fits_precision(const unsigned long long (&mag)[N], const unsigned long long (&pow10_p)[N]) {
  return dec_less<N>(mag, pow10_p);
}

// w · 10^k mod 2^(64N), k ≥ 0.  Returns whether a carry left the top limb: on a magnitude, the product does not fit the width; on a
// two's complement value the low limbs are the wrapped product and the return value means nothing.
template <int N>
AH_DEC_FN bool dec_mul_pow10(unsigned long long (&w)[N], int k) {
  unsigned long long lost = 0;
  while (k > 0) {
    const unsigned long long m = kPow10[k < 19 ? k : 19];
    k -= 19;
    unsigned long long carry = 0;
#pragma unroll
    for (int t = 0; t < N; t++) {
      const unsigned __int128 p = (unsigned __int128)w[t] * m + carry;
      w[t] = (unsigned long long)p;
      carry = (unsigned long long)(p >> 64);
    }
    lost |= carry;
  }
  return lost != 0;
}

// (u1 · 2^64 + u0) / d for a normalised d (bit 63 set), u1 < d, with v = ⌊(2^128 − 1) / d⌋ − 2^64: quotient, *r = remainder
AH_DEC_FN unsigned long long dec_div_2by1(unsigned long long u1, unsigned long long u0, unsigned long long d, unsigned long long v,
                                          unsigned long long* r) {
  const unsigned __int128 q = (unsigned __int128)v * u1 + (((unsigned __int128)u1 << 64) | u0);
  unsigned long long q1 = (unsigned long long)(q >> 64) + 1;
  const unsigned long long q0 = (unsigned long long)q;
  unsigned long long rem = u0 - q1 * d;
  if (rem > q0) { q1--; rem += d; }
  if (rem >= d) { q1++; rem -= d; }
  *r = rem;
  return q1;
}

// w = ⌊w / 10^j⌋ for one step 1 ≤ j ≤ 19 (unsigned); returns the remainder
template <int N>
AH_DEC_FN unsigned long long dec_div_step(unsigned long long (&w)[N], int j) {
  const unsigned long long d = kPow10Norm[j], v = kPow10Recip[j];
  const int s = kPow10Shift[j];
  // the dividend shifted left by s takes N + 1 limbs; its top limb (< 2^s ≤ d) is the first partial remainder
  unsigned long long r = s ? w[N - 1] >> (64 - s) : 0;
#pragma unroll
  for (int t = N - 1; t >= 0; t--) {
    const unsigned long long below = t > 0 ? w[t - 1] : 0;
    const unsigned long long u0 = s ? (w[t] << s) | (below >> (64 - s)) : w[t];
    w[t] = dec_div_2by1(r, u0, d, v, &r);
  }
  return r >> s;
}

// Truncated division of a magnitude: q = ⌊x / 10^k⌋, k ≥ 0.  *rem_nonzero: x is not a multiple of 10^k (Rescale's "data loss",
// decimal128.go:468-477); *half_or_more: 2·(x − q·10^k) ≥ 10^k (ReduceScaleBy's rounding test, :459-463) — from r = x − q·10^k.
// HALF = false leaves *half_or_more alone and takes the remainder test from the steps' remainders.
template <int N, bool HALF>
AH_DEC_FN void dec_div_pow10(const unsigned long long (&x)[N], int k, unsigned long long (&q)[N], bool* rem_nonzero, bool* half_or_more) {
#pragma unroll
  for (int t = 0; t < N; t++) q[t] = x[t];
  unsigned long long any = 0;
  int left = k;
  while (left > 0) {
    const int j = left < 19 ? left : 19;
    left -= 19;
    any |= dec_div_step<N>(q, j);
  }
  *rem_nonzero = any != 0;
  if constexpr (HALF) {
    // r = x − q·10^k < 10^k; k ≤ 76 keeps 2r and 10^k below 2^256, k ≤ 38 below 2^128
    unsigned long long p[N], r[N], den[N];
#pragma unroll
    for (int t = 0; t < N; t++) { p[t] = q[t]; den[t] = t == 0 ? 1 : 0; }
    dec_mul_pow10<N>(p, k);
    dec_mul_pow10<N>(den, k);
    unsigned long long borrow = 0;
#pragma unroll
    for (int t = 0; t < N; t++) {
      const unsigned long long a = x[t], b = p[t];
      const unsigned long long d1 = a - b;
      const unsigned long long d2 = d1 - borrow;
      borrow = (a < b || d1 < borrow) ? 1 : 0;
      r[t] = d2;
    }
    // 2r
    unsigned long long top = 0;
#pragma unroll
    for (int t = 0; t < N; t++) {
      const unsigned long long v = (r[t] << 1) | top;
      top = r[t] >> 63;
      r[t] = v;
    }
    *half_or_more = k > 0 && !dec_less<N>(r, den);
  }
}

// magnitude + 1 (ReduceScaleBy's result.Add(result, sign): one away from zero)
template <int N>
AH_DEC_FN void dec_increment(unsigned long long (&w)[N]) {
  unsigned long long carry = 1;
#pragma unroll
  for (int t = 0; t < N; t++) {
    w[t] += carry;
    carry = (carry && w[t] == 0) ? 1 : 0;
  }
}

#if defined(__HIPCC__)
// the value of a W-byte slot in N limbs (N·8 ≥ W: sign-extended), 16 bytes per load
template <int N, int W>
__device__ __forceinline__ void dec_load(const uint8_t* p, unsigned long long (&w)[N]) {
  static_assert(N * 8 >= W && (W == 16 || W == 32) && (N == 2 || N == 4), "decimal slot does not fit the limbs");
  const V2u64 lo = reinterpret_cast<const V2u64u*>(p)->v;
  w[0] = lo.x;
  w[1] = lo.y;
  if constexpr (N == 4) {
    if constexpr (W == 32) {
      const V2u64 hi = reinterpret_cast<const V2u64u*>(p + 16)->v;
      w[2] = hi.x;
      w[3] = hi.y;
    } else {
      w[2] = w[3] = (unsigned long long)((long long)w[1] >> 63);
    }
  }
}

// the low W bytes of N limbs (N = 2 into a 32-byte slot: sign-extended), 16 bytes per store
template <int N, int W>
__device__ __forceinline__ void dec_store(uint8_t* p, const unsigned long long (&w)[N]) {
  static_assert((W == 16 || W == 32) && (N == 2 || N == 4), "decimal slot width");
  V2u64 lo;
  lo.x = w[0];
  lo.y = w[1];
  reinterpret_cast<V2u64u*>(p)->v = lo;
  if constexpr (W == 32) {
    V2u64 hi;
    if constexpr (N == 4) { hi.x = w[2]; hi.y = w[3]; }
    else { hi.x = hi.y = (unsigned long long)((long long)w[1] >> 63); }
    reinterpret_cast<V2u64u*>(p + 16)->v = hi;
  }
}
#endif
