// ah_cast_decimal.hip — the decimal casts: decimal → decimal (rescale, change of precision and width), integer → decimal,
// decimal → integer.
//
// Replaces CastDecimalToDecimal (arrow/compute/internal/kernels/numeric_cast.go:377-429: safeRescaleDecimal128Out / 256Out :310-375,
// unsafeUpscale* / unsafeDownscale* :264-308), CastIntegerToDecimal (:173-239) and CastDecimal128ToInteger / CastDecimal256ToInteger
// (:79-171) behind compute's "cast".  All arithmetic is on the unscaled integer, in the limbs of ah_decimal.h.
//
// One pass, one row per lane, 16 bytes per load and store.  ScalarUnaryNotNull: a null slot is not read (whatever lies under it cannot
// fail) and its output is zero bytes; the validity word of a wave's 64 rows is one scalar load.  Conversion, check and the report of
// the FIRST offending row happen in that pass, as in ah_cast_impl.h: an offender does atomicMin(row · 4 + reason) on one device word,
// which the host reads once when a check was active.
//
// Where a product leaves the width (the reference's FromBigInt panics there, decimal128.go:78-82): a checked cast computes on the
// magnitude, sees the carry out of the top limb and reports "does not fit in precision"; an unchecked one wraps modulo 2^128 / 2^256
// (what Arrow C++ returns) — DESIGN.md "Reference quirks — decisions".
#include "ah_common.h"
#include "ah_decimal.h"

namespace {

constexpr int kBlock = 256;
enum { kUp = 1, kDown = 2 };                       // MODE: 0 = the scale stays
enum { kLoss = 1, kNoFit = 2, kOutOfBounds = 3 };  // reasons, in the order one row meets them

template <int N> struct Limbs { unsigned long long w[N]; };

__device__ __forceinline__ void report(unsigned long long& bad_at, int64_t row, int reason) {
  const unsigned long long at = ((unsigned long long)row << 2) | (unsigned)reason;
  if (at < bad_at) bad_at = at;
}

// decimal → decimal.  N: limbs of the working value.  SAFE: data-loss and precision checks on; else truncate / wrap.
template <int WIN, int WOUT, int N, int MODE, bool SAFE>
__global__ __launch_bounds__(kBlock) void rescale_kernel(const uint8_t* __restrict__ in, const uint8_t* __restrict__ valid, int64_t off, int64_t n,
                                                         uint8_t* __restrict__ out, int k, Limbs<N> bound, unsigned long long* __restrict__ first_bad) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  unsigned long long bad_at = ~0ull;
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const unsigned long long vword = valid ? ah_wave_bits64(valid, off + ch * 64, left) : ~0ull;
    if (lane >= left) continue;
    unsigned long long w[N];
#pragma unroll
    for (int t = 0; t < N; t++) w[t] = 0;
    if ((vword >> lane) & 1) {
      dec_load<N, WIN>(in + row * WIN, w);
      if constexpr (SAFE || MODE == kDown) {
        const bool neg = dec_is_negative<N>(w);
        if (neg) dec_negate<N>(w);
        int reason = 0;
        if constexpr (MODE == kUp) {
          if (dec_mul_pow10<N>(w, k) && SAFE) reason = kNoFit;
        } else if constexpr (MODE == kDown) {
          bool nonzero, half;
          unsigned long long q[N];
          dec_div_pow10<N, false>(w, k, q, &nonzero, &half);
#pragma unroll
          for (int t = 0; t < N; t++) w[t] = q[t];
          if (SAFE && nonzero) reason = kLoss;
        }
        if (SAFE && reason == 0 && !dec_fits_precision<N>(w, bound.w)) reason = kNoFit;
        if (neg) dec_negate<N>(w);
        if (SAFE && reason) report(bad_at, row, reason);
      } else if constexpr (MODE == kUp) {
        dec_mul_pow10<N>(w, k);  // two's complement: the low limbs are the wrapped product
      }
    }
    dec_store<N, WOUT>(out + row * WOUT, w);
  }
  if (SAFE && bad_at != ~0ull) atomicMin(first_bad, bad_at);
}

// integer → decimal: value · 10^scale, which the precision check (made from the types) keeps inside the width
template <typename T, int WOUT>
__global__ __launch_bounds__(kBlock) void int_to_decimal_kernel(const T* __restrict__ in, const uint8_t* __restrict__ valid, int64_t off, int64_t n,
                                                                uint8_t* __restrict__ out, int k) {
  constexpr int N = WOUT / 8;
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const unsigned long long vword = valid ? ah_wave_bits64(valid, off + ch * 64, left) : ~0ull;
    if (lane >= left) continue;
    unsigned long long w[N];
#pragma unroll
    for (int t = 0; t < N; t++) w[t] = 0;
    if ((vword >> lane) & 1) {
      const T v = in[row];
      w[0] = (unsigned long long)v;  // sign- or zero-extended by T's signedness
      const unsigned long long ext = v < 0 ? ~0ull : 0ull;
#pragma unroll
      for (int t = 1; t < N; t++) w[t] = ext;
      if (k) dec_mul_pow10<N>(w, k);
    }
    dec_store<N, WOUT>(out + row * WOUT, w);
  }
}

// decimal → integer of B bytes.  MODE kDown: ÷ 10^k (k = the input's scale); kUp: × 10^k (a negative scale).  safe: a non-zero
// remainder is data loss; else the quotient is rounded half away from zero (ReduceScaleBy(scale, true)).  check_range: the value must
// lie in [lo, hi] (lo as a signed, hi as an unsigned 64-bit number).  The result is the low 64 bits narrowed to B bytes.
template <int WIN, int N, int B, int MODE>
__global__ __launch_bounds__(kBlock) void decimal_to_int_kernel(const uint8_t* __restrict__ in, const uint8_t* __restrict__ valid, int64_t off, int64_t n,
                                                                uint8_t* __restrict__ out, int k, int safe, int check_range, long long lo,
                                                                unsigned long long hi, unsigned long long* __restrict__ first_bad) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  unsigned long long bad_at = ~0ull;
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const unsigned long long vword = valid ? ah_wave_bits64(valid, off + ch * 64, left) : ~0ull;
    if (lane >= left) continue;
    unsigned long long res = 0;
    if ((vword >> lane) & 1) {
      unsigned long long w[N];
      dec_load<N, WIN>(in + row * WIN, w);
      int reason = 0;
      bool beyond = false;  // the scaled value left the working width
      if constexpr (MODE != 0) {
        const bool neg = dec_is_negative<N>(w);
        if (neg) dec_negate<N>(w);
        if constexpr (MODE == kUp) {
          beyond = dec_mul_pow10<N>(w, k);
          // a magnitude with its top bit set has no two's complement of its sign, −2^(64N−1) aside
          bool low_zero = true;
#pragma unroll
          for (int t = 0; t < N - 1; t++) low_zero = low_zero && w[t] == 0;
          if ((long long)w[N - 1] < 0 && !(neg && low_zero && w[N - 1] == 1ull << 63)) beyond = true;
        } else {
          bool nonzero, half;
          unsigned long long q[N];
          dec_div_pow10<N, true>(w, k, q, &nonzero, &half);
#pragma unroll
          for (int t = 0; t < N; t++) w[t] = q[t];
          if (safe) { if (nonzero) reason = kLoss; }
          else if (half) dec_increment<N>(w);
        }
        if (neg) dec_negate<N>(w);
      }
      if (check_range && reason == 0) {
        const bool neg = dec_is_negative<N>(w);
        bool upper_ok = true;
#pragma unroll
        for (int t = 1; t < N; t++) upper_ok = upper_ok && w[t] == (neg ? ~0ull : 0ull);
        const bool in_range = neg ? (upper_ok && (long long)w[0] < 0 && (long long)w[0] >= lo) : (upper_ok && w[0] <= hi);
        if (beyond || !in_range) reason = kOutOfBounds;
      }
      if (reason) report(bad_at, row, reason);
      else res = w[0];
    }
    uint8_t* o = out + row * B;
    if constexpr (B == 1) *o = (uint8_t)res;
    else if constexpr (B == 2) *(uint16_t*)o = (uint16_t)res;
    else if constexpr (B == 4) *(uint32_t*)o = (uint32_t)res;
    else *(unsigned long long*)o = res;
  }
  if (bad_at != ~0ull) atomicMin(first_bad, bad_at);
}

unsigned chunk_grid(ah_ctx* c, int64_t n) { return ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, 64), kBlock / 64), 8); }

// 10^p in N limbs (p ≤ 38 for N = 2, ≤ 76 for N = 4)
template <int N>
Limbs<N> pow10_limbs(int p) {
  Limbs<N> b;
  for (int t = 0; t < N; t++) b.w[t] = t == 0 ? 1 : 0;
  for (int i = 0; i < p; i++) {
    unsigned long long carry = 0;
    for (int t = 0; t < N; t++) {
      const unsigned __int128 v = (unsigned __int128)b.w[t] * 10 + carry;
      b.w[t] = (unsigned long long)v;
      carry = (unsigned long long)(v >> 64);
    }
  }
  return b;
}

int arm_first_bad(ah_ctx* c) {
  AH_HIP(c, hipMemsetAsync(&c->dscalars[12], 0xFF, sizeof(uint64_t), c->stream));
  return AH_OK;
}

// the first offender of a checked cast, as the reference's error
int read_first_bad(ah_ctx* c) {
  AH_HIP(c, hipMemcpyAsync(c->pinned, &c->dscalars[12], sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipStreamSynchronize(c->stream));
  const unsigned long long at = *(volatile unsigned long long*)c->pinned;
  if (at == ~0ull) return AH_OK;
  switch ((int)(at & 3)) {
    case kLoss: return ah_fail(c, AH_EINVALID, "rescale data loss");                                  // decimal128.go:506
    case kNoFit: return ah_fail(c, AH_EINVALID, "decimal value does not fit in precision");           // numeric_cast.go:323
    default: return ah_fail(c, AH_EINVALID, "integer value out of bounds");                           // numeric_cast.go:85
  }
}

template <int WIN, int WOUT, int N>
void launch_rescale(ah_ctx* c, const uint8_t* in, const uint8_t* valid, int64_t off, int64_t n, uint8_t* out, int delta, int out_precision,
                    bool safe) {
  const unsigned grid = chunk_grid(c, n);
  unsigned long long* fb = (unsigned long long*)&c->dscalars[12];
  const int k = delta < 0 ? -delta : delta;
  const Limbs<N> bound = pow10_limbs<N>(safe ? out_precision : 0);
#define AH_RESCALE(MODE, SAFE) rescale_kernel<WIN, WOUT, N, MODE, SAFE><<<grid, kBlock, 0, c->stream>>>(in, valid, off, n, out, k, bound, fb)
  if (delta > 0) { if (safe) AH_RESCALE(kUp, true); else AH_RESCALE(kUp, false); }
  else if (delta < 0) { if (safe) AH_RESCALE(kDown, true); else AH_RESCALE(kDown, false); }
  else { if (safe) AH_RESCALE(0, true); else AH_RESCALE(0, false); }
#undef AH_RESCALE
}

template <typename T>
void launch_int_to_decimal(ah_ctx* c, int out_width, const void* in, const uint8_t* valid, int64_t off, int64_t n, uint8_t* out, int scale) {
  const unsigned grid = chunk_grid(c, n);
  if (out_width == 16) int_to_decimal_kernel<T, 16><<<grid, kBlock, 0, c->stream>>>((const T*)in, valid, off, n, out, scale);
  else int_to_decimal_kernel<T, 32><<<grid, kBlock, 0, c->stream>>>((const T*)in, valid, off, n, out, scale);
}

template <int WIN, int B>
void launch_decimal_to_int(ah_ctx* c, const uint8_t* in, const uint8_t* valid, int64_t off, int64_t n, uint8_t* out, int in_scale, int safe,
                           int check_range, long long lo, unsigned long long hi) {
  const unsigned grid = chunk_grid(c, n);
  unsigned long long* fb = (unsigned long long*)&c->dscalars[12];
  if (in_scale > 0)
    decimal_to_int_kernel<WIN, WIN / 8, B, kDown><<<grid, kBlock, 0, c->stream>>>(in, valid, off, n, out, in_scale, safe, check_range, lo, hi, fb);
  else if (in_scale < 0)
    decimal_to_int_kernel<WIN, 4, B, kUp><<<grid, kBlock, 0, c->stream>>>(in, valid, off, n, out, -in_scale, safe, check_range, lo, hi, fb);
  else
    decimal_to_int_kernel<WIN, WIN / 8, B, 0><<<grid, kBlock, 0, c->stream>>>(in, valid, off, n, out, 0, safe, check_range, lo, hi, fb);
}

template <int WIN>
int decimal_to_int_width(ah_ctx* c, int bytes, const uint8_t* in, const uint8_t* valid, int64_t off, int64_t n, uint8_t* out, int in_scale, int safe,
                         int check_range, long long lo, unsigned long long hi) {
  switch (bytes) {
    case 1: launch_decimal_to_int<WIN, 1>(c, in, valid, off, n, out, in_scale, safe, check_range, lo, hi); break;
    case 2: launch_decimal_to_int<WIN, 2>(c, in, valid, off, n, out, in_scale, safe, check_range, lo, hi); break;
    case 4: launch_decimal_to_int<WIN, 4>(c, in, valid, off, n, out, in_scale, safe, check_range, lo, hi); break;
    default: launch_decimal_to_int<WIN, 8>(c, in, valid, off, n, out, in_scale, safe, check_range, lo, hi); break;
  }
  return AH_OK;
}

// bytes, signedness and MaxDecimalDigitsForInt (kernels/helpers.go:705-719) of an integer type id; false: not an integer
bool int_type(int t, int* bytes, bool* is_signed, int* digits) {
  switch (t) {
    case AH_UINT8: *bytes = 1; *is_signed = false; *digits = 3; return true;
    case AH_INT8: *bytes = 1; *is_signed = true; *digits = 3; return true;
    case AH_UINT16: *bytes = 2; *is_signed = false; *digits = 5; return true;
    case AH_INT16: *bytes = 2; *is_signed = true; *digits = 5; return true;
    case AH_UINT32: *bytes = 4; *is_signed = false; *digits = 10; return true;
    case AH_INT32: *bytes = 4; *is_signed = true; *digits = 10; return true;
    case AH_UINT64: *bytes = 8; *is_signed = false; *digits = 20; return true;
    case AH_INT64: *bytes = 8; *is_signed = true; *digits = 19; return true;
  }
  return false;
}

int check_column(ah_ctx* c, const char* what, const void* values, int64_t off, int64_t n, const void* out) {
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "%s: negative length/offset", what);
  if (n > 0 && (!values || !out)) return ah_fail(c, AH_EINVALID, "%s: null buffer", what);
  return AH_OK;
}

}  // namespace

AH_EXPORT int ah_cast_decimal_rescale(ah_ctx* c, int in_width, int out_width, int scale_delta, int out_precision, int allow_truncate,
                                      const void* values, const uint8_t* valid, int64_t off, int64_t n, void* out_values) {
  AH_ENTER(c);
  int rc = check_column(c, "decimal cast", values, off, n, out_values);
  if (rc != AH_OK) return rc;
  if ((in_width != 16 && in_width != 32) || (out_width != 16 && out_width != 32))
    return ah_fail(c, AH_EINVALID, "decimal cast: width must be 16 or 32 (got %d, %d)", in_width, out_width);
  if (scale_delta < -76 || scale_delta > 76) return ah_fail(c, AH_EINVALID, "decimal cast: scale change must be −76 … 76 (got %d)", scale_delta);
  const bool safe = !allow_truncate;
  const int max_p = out_width == 16 ? 38 : 76;
  if (safe && (out_precision < 1 || out_precision > max_p))
    return ah_fail(c, AH_EINVALID, "decimal cast: precision must be 1 … %d (got %d)", max_p, out_precision);
  if (n == 0) return AH_OK;
  if (safe) { rc = arm_first_bad(c); if (rc != AH_OK) return rc; }
  const uint8_t* in = (const uint8_t*)values;
  uint8_t* out = (uint8_t*)out_values;
  const bool narrow_work = scale_delta >= -38 && scale_delta <= 38;  // 128 → 128: two limbs carry every step
  if (in_width == 16 && out_width == 16) {
    if (narrow_work) launch_rescale<16, 16, 2>(c, in, valid, off, n, out, scale_delta, out_precision, safe);
    else launch_rescale<16, 16, 4>(c, in, valid, off, n, out, scale_delta, out_precision, safe);
  } else if (in_width == 16) launch_rescale<16, 32, 4>(c, in, valid, off, n, out, scale_delta, out_precision, safe);
  else if (out_width == 16) launch_rescale<32, 16, 4>(c, in, valid, off, n, out, scale_delta, out_precision, safe);
  else launch_rescale<32, 32, 4>(c, in, valid, off, n, out, scale_delta, out_precision, safe);
  AH_LAUNCH_CHECK(c);
  return safe ? read_first_bad(c) : AH_OK;
}

AH_EXPORT int ah_cast_int_to_decimal(ah_ctx* c, int in_type, int out_width, int scale, const void* values, const uint8_t* valid, int64_t off,
                                     int64_t n, void* out_values) {
  AH_ENTER(c);
  int rc = check_column(c, "integer to decimal cast", values, off, n, out_values);
  if (rc != AH_OK) return rc;
  int bytes = 0, digits = 0;
  bool is_signed = false;
  if (!int_type(in_type, &bytes, &is_signed, &digits)) return ah_fail(c, AH_EINVALID, "integer to decimal cast: type %d is not an integer", in_type);
  if (out_width != 16 && out_width != 32) return ah_fail(c, AH_EINVALID, "integer to decimal cast: width must be 16 or 32 (got %d)", out_width);
  if (scale < 0) return ah_fail(c, AH_EINVALID, "scale must be non-negative");  // numeric_cast.go:223-225
  const int max_p = out_width == 16 ? 38 : 76;
  if (digits + scale > max_p)  // the caller's precision check (numeric_cast.go:227-236) implies this: the product cannot leave the width
    return ah_fail(c, AH_EINVALID, "precision is not great enough for result. It should be at least %d", digits + scale);
  if (n == 0) return AH_OK;
  const uint8_t* in = (const uint8_t*)values;
  uint8_t* out = (uint8_t*)out_values;
  switch (in_type) {
    case AH_UINT8: launch_int_to_decimal<uint8_t>(c, out_width, in, valid, off, n, out, scale); break;
    case AH_INT8: launch_int_to_decimal<int8_t>(c, out_width, in, valid, off, n, out, scale); break;
    case AH_UINT16: launch_int_to_decimal<uint16_t>(c, out_width, in, valid, off, n, out, scale); break;
    case AH_INT16: launch_int_to_decimal<int16_t>(c, out_width, in, valid, off, n, out, scale); break;
    case AH_UINT32: launch_int_to_decimal<uint32_t>(c, out_width, in, valid, off, n, out, scale); break;
    case AH_INT32: launch_int_to_decimal<int32_t>(c, out_width, in, valid, off, n, out, scale); break;
    case AH_UINT64: launch_int_to_decimal<uint64_t>(c, out_width, in, valid, off, n, out, scale); break;
    default: launch_int_to_decimal<int64_t>(c, out_width, in, valid, off, n, out, scale); break;
  }
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

AH_EXPORT int ah_cast_decimal_to_int(ah_ctx* c, int in_width, int in_scale, int out_type, int allow_truncate, int allow_overflow,
                                     const void* values, const uint8_t* valid, int64_t off, int64_t n, void* out_values) {
  AH_ENTER(c);
  int rc = check_column(c, "decimal to integer cast", values, off, n, out_values);
  if (rc != AH_OK) return rc;
  int bytes = 0, digits = 0;
  bool is_signed = false;
  if (!int_type(out_type, &bytes, &is_signed, &digits)) return ah_fail(c, AH_EINVALID, "decimal to integer cast: type %d is not an integer", out_type);
  if (in_width != 16 && in_width != 32) return ah_fail(c, AH_EINVALID, "decimal to integer cast: width must be 16 or 32 (got %d)", in_width);
  const int max_s = in_width == 16 ? 38 : 76;
  if (in_scale < -max_s || in_scale > max_s) return ah_fail(c, AH_EINVALID, "decimal to integer cast: scale must be −%d … %d (got %d)", max_s, max_s, in_scale);
  if (n == 0) return AH_OK;
  rc = arm_first_bad(c);
  if (rc != AH_OK) return rc;
  // MinOf / MaxOf of the target (numeric_cast.go:97-105, 138-146), both inclusive
  const int bits = bytes * 8;
  const long long lo = is_signed ? (bits == 64 ? INT64_MIN : -(1ll << (bits - 1))) : 0;
  const unsigned long long hi = is_signed ? (unsigned long long)((1ull << (bits - 1)) - 1) : (bits == 64 ? ~0ull : (1ull << bits) - 1);
  const uint8_t* in = (const uint8_t*)values;
  const int safe = allow_truncate ? 0 : 1, check_range = allow_overflow ? 0 : 1;
  if (in_width == 16) decimal_to_int_width<16>(c, bytes, in, valid, off, n, (uint8_t*)out_values, in_scale, safe, check_range, lo, hi);
  else decimal_to_int_width<32>(c, bytes, in, valid, off, n, (uint8_t*)out_values, in_scale, safe, check_range, lo, hi);
  AH_LAUNCH_CHECK(c);
  // nothing can fail when a zero scale meets an unchecked range — the read is skipped there
  if (!check_range && (in_scale <= 0 || !safe)) return AH_OK;
  return read_first_bad(c);
}
