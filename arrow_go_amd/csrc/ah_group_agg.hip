// ah_group_agg.hip — the aggregates over caller-supplied dense group ids for value columns of every numeric width, the count that reads
// no values, the mean, and the second moment about the mean: ah_group_sum_typed, ah_group_min_max_typed, ah_group_count, ah_group_mean,
// ah_group_m2, ah_group_variance.
//
// No reference analogue (arrow-go has no hash aggregate); definitions in DESIGN.md §3.2.  These sit BESIDE ah_hash_agg.hip, whose
// kernels read 8-byte values only and are left as they are: a caller holding an Int32 or Float32 column had to write an 8-byte copy of
// it to HBM first.  Here a value is loaded at its own width where it lies (element-aligned: an Int8 slice at offset 3 is fine) and
// widened in registers — sign-extended, zero-extended or converted to double — to the 64-bit word the 8-byte aggregate would have read,
// so THE BYTES of every result are those of ah_group_sum_* / ah_group_min_max_* on the cast column:
//   · integer sums wrap in 64 bits, and 64-bit addition commutes;
//   · Float32 sums go through the 128-bit fixed-point accumulation of ah_hashing.h, which is exact and therefore independent of order
//     and launch geometry; the scale comes from a typed absmax pass over the widened values, the wide-column route (a scale per group)
//     and the non-finite flags are the same;
//   · min / max are atomicMin / atomicMax on the order-preserving words of ah_group_order.h; narrowing the 64-bit result back to the
//     input type is exact because every candidate came from that type.
// The 8-byte types forward to the existing entry points.
//
// ONE skeleton, typed_agg_kernel<Agg, T, USE_LDS>, with the regimes of ah_hash_agg.hip: up to 4096 groups every workgroup keeps all
// groups in LDS (a 32-bit count per group plus the policy's 64-bit words: 16 ... 80 KiB, two workgroups per CU) and flushes the touched
// ones once; above that, device atomics straight into the accumulators with the same bounds check (the narrow types do NOT take the
// partitioned pair stream of the 8-byte sum: it would write the widened column this file exists to avoid).
// HBM: 4 B/row of ids + the value at its own width + the validity bits; the count reads no values.
//
// ah_group_m2 reads a column of any of the ten types as cast to Float64 and makes three or four passes over it: the sum behind the
// mean, the scale of the squared deviations, their fixed-point accumulation.  Its policies (GroupScale, ScaledSum) run in a kernel of
// their own, cast_agg_kernel: the skeleton over again, with the cast and with the per-group words a row needs (the mean, the scale)
// gathered for a whole step in front of the row loop.  typed_agg_kernel and its launch are not touched by it, so what the existing
// instantiations compile to is what it was.
#include "ah_common.h"
#include "ah_hashing.h"
#include "ah_group_order.h"

namespace {

constexpr int kTypedLdsGroups = 4096;
constexpr unsigned kQuietNaN32 = 0x7FC00000u;

// the 64-bit word the 8-byte aggregate reads for this value: Int64 / UInt64 bit pattern, or the bits of the double
template <typename T>
__device__ __forceinline__ unsigned long long widen(T v) {
  if constexpr (std::is_same<T, float>::value) return __builtin_bit_cast(unsigned long long, (double)v);
  else if constexpr (std::is_signed<T>::value) return (unsigned long long)(long long)v;
  else return (unsigned long long)v;
}
template <typename T>
constexpr int kind_of() { return std::is_same<T, float>::value ? kF64 : std::is_signed<T>::value ? kI64 : kU64; }

// ---- the policies (the shape of ah_hash_agg.hip's: kWords 64-bit LDS words per group, word j of slot l is w[j · kTypedLdsGroups + l]) ----
struct CountRows {   // the skeleton's own count is the whole aggregate
  static constexpr int kWords = 0;
  static constexpr bool kReads = false, kCounts = true;
  __device__ static constexpr unsigned long long identity(int) { return 0; }
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void row_lds(unsigned long long*, int, size_t, unsigned long long) const {}
  __device__ __forceinline__ void row_global(size_t, unsigned long long) const {}
  __device__ __forceinline__ void flush(const unsigned long long*, int, size_t) const {}
};

struct WidenedSumInt {
  static constexpr int kWords = 1;
  static constexpr bool kReads = true, kCounts = true;
  unsigned long long* sums;
  __device__ static constexpr unsigned long long identity(int) { return 0; }
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void row_lds(unsigned long long* w, int l, size_t, unsigned long long bits) const { atomicAdd(&w[l], bits); }
  __device__ __forceinline__ void row_global(size_t g, unsigned long long bits) const { atomicAdd(&sums[g], bits); }
  __device__ __forceinline__ void flush(const unsigned long long* w, int l, size_t g) const { atomicAdd(&sums[g], w[l]); }
};

struct WidenedSumFloat {   // fx.gmax set (wide columns): the group's own scale, looked up per row
  static constexpr int kWords = 2;
  static constexpr bool kReads = true, kCounts = true;
  FxAcc fx;
  int sh;
  __device__ static constexpr unsigned long long identity(int) { return 0; }
  __device__ __forceinline__ void begin() { sh = fx_shift(*fx.absmax); }
  __device__ __forceinline__ void add(unsigned long long* lo_arr, unsigned long long* hi_arr, size_t slot, size_t g, unsigned long long bits) const {
    const double x = __builtin_bit_cast(double, bits);
    if (fx_finite(x)) {
      unsigned long long lo, hi;
      fx_split(x, fx.gmax ? fx_shift(fx.gmax[g]) : sh, &lo, &hi);
      fx_add(lo_arr, hi_arr, slot, lo, hi);
    } else {
      atomicOr(&fx.flags[g], fx_flag(x));
    }
  }
  __device__ __forceinline__ void row_lds(unsigned long long* w, int l, size_t g, unsigned long long bits) const { add(w, w + kTypedLdsGroups, (size_t)l, g, bits); }
  __device__ __forceinline__ void row_global(size_t g, unsigned long long bits) const { add(fx.lo, fx.hi, g, g, bits); }
  __device__ __forceinline__ void flush(const unsigned long long* w, int l, size_t g) const { fx_add(fx.lo, fx.hi, g, w[l], w[kTypedLdsGroups + l]); }
};

template <int KIND>
struct WidenedMinMax {   // mins / maxs (64-bit ordered words, temporaries) hold the identities, the counts zeros, when the aggregate starts
  static constexpr int kWords = 2;
  static constexpr bool kReads = true, kCounts = true;
  unsigned long long *mins, *maxs;
  __device__ static constexpr unsigned long long identity(int j) { return j == 0 ? kMinIdentity : kMaxIdentity; }
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void row_lds(unsigned long long* w, int l, size_t, unsigned long long bits) const {
    if (is_nan_bits<KIND>(bits)) return;
    const unsigned long long x = to_ordered<KIND>(bits);
    if (x < look_lds(&w[l])) atomicMin(&w[l], x);
    if (x > look_lds(&w[kTypedLdsGroups + l])) atomicMax(&w[kTypedLdsGroups + l], x);
  }
  __device__ __forceinline__ void row_global(size_t g, unsigned long long bits) const {
    if (is_nan_bits<KIND>(bits)) return;
    const unsigned long long x = to_ordered<KIND>(bits);
    if (x < look(&mins[g])) atomicMin(&mins[g], x);
    if (x > look(&maxs[g])) atomicMax(&maxs[g], x);
  }
  __device__ __forceinline__ void flush(const unsigned long long* w, int l, size_t g) const {
    const unsigned long long lo = w[l], hi = w[kTypedLdsGroups + l];
    if (lo < look(&mins[g])) atomicMin(&mins[g], lo);
    if (hi > look(&maxs[g])) atomicMax(&maxs[g], hi);
  }
};

struct WidenedAbsMax {   // wide Float32 columns: largest finite |x| per group, as the bits of the double.  Global only, nothing counted.
  static constexpr int kWords = 0;
  static constexpr bool kReads = true, kCounts = false;
  unsigned long long* gmax;   // zeros when the aggregate starts
  __device__ static constexpr unsigned long long identity(int) { return 0; }
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void row_lds(unsigned long long*, int, size_t, unsigned long long) const {}
  __device__ __forceinline__ void row_global(size_t g, unsigned long long bits) const {
    const unsigned long long a = bits & ~kSignBit;
    if ((a >> 52) == 0x7ff || a == 0) return;
    if (look(&gmax[g]) < a) atomicMax(&gmax[g], a);
  }
  __device__ __forceinline__ void flush(const unsigned long long*, int, size_t) const {}
};

// ---- the skeleton ------------------------------------------------------------------------------------------------------------------
// USE_LDS: ngroups ≤ kTypedLdsGroups (the host's choice).  An id outside [0, ngroups) fails the one unsigned comparison in front of
// every access to a group's words: such a row touches neither LDS nor HBM.
template <typename Agg, typename T, bool USE_LDS>
__global__ __launch_bounds__(kBlock) void typed_agg_kernel(const int32_t* __restrict__ ids, const T* __restrict__ vals, const uint8_t* __restrict__ vvalid,
                                                            int64_t voff, int64_t n, unsigned long long* __restrict__ counts, int ngroups, Agg agg) {
  __shared__ unsigned long long s_w[USE_LDS && Agg::kWords > 0 ? Agg::kWords * kTypedLdsGroups : 1];
  __shared__ unsigned s_cnt[USE_LDS ? kTypedLdsGroups : 1];
  const int nl = USE_LDS && ngroups > kTypedLdsGroups ? kTypedLdsGroups : ngroups;
  if constexpr (USE_LDS) {
    for (int l = threadIdx.x; l < nl; l += kBlock) {
#pragma unroll
      for (int j = 0; j < Agg::kWords; j++) s_w[j * kTypedLdsGroups + l] = Agg::identity(j);
      s_cnt[l] = 0;
    }
    __syncthreads();
  }
  agg.begin();
  // Rows per lane per step: 8 id loads + 8 value loads (+ 8 validity bytes) in flight.  All of them are UNCONDITIONAL, from a row index
  // clamped to n − 1, and a value stays as loaded until the second loop: with the loads under `ok ? load : 0` the widening (a sign
  // extension, a conversion) was placed right behind its load inside the masked block, so every value was waited for before the next
  // load went out — 2.2 x the time of the 8-byte kernel for half the bytes (measured).  The payload under a null is loaded and dropped.
  // The loop exists twice, with and without a validity bitmap (wave-uniform), so that neither has a branch between its loads.
  constexpr int U = 8;
  const int64_t stride = (int64_t)gridDim.x * kBlock * U;
  auto rows = [&](auto has_valid) {
    for (int64_t base = (int64_t)blockIdx.x * kBlock * U + threadIdx.x; base < n; base += stride) {
      int32_t g[U];
      T raw[U];
      uint8_t vb[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int64_t i = base + (int64_t)u * kBlock, ic = i < n ? i : n - 1;
        g[u] = __builtin_nontemporal_load(&ids[ic]);
        if constexpr (Agg::kReads) raw[u] = __builtin_nontemporal_load(&vals[ic]);
        else raw[u] = T(0);
        if constexpr (decltype(has_valid)::value) vb[u] = vvalid[(voff + ic) >> 3];
        else vb[u] = 0xff;
      }
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int64_t i = base + (int64_t)u * kBlock;
        const bool ok = i < n && ((vb[u] >> ((voff + i) & 7)) & 1);
        // a null value, a row past the end, or an id that is not a group's: out of memory the call does not own
        if (!ok || (unsigned)g[u] >= (unsigned)nl) continue;
        const unsigned long long v = Agg::kReads ? widen<T>(raw[u]) : 0ull;
        if constexpr (USE_LDS) {
          agg.row_lds(s_w, g[u], (size_t)g[u], v);
          atomicAdd(&s_cnt[g[u]], 1u);
        } else {
          agg.row_global((size_t)g[u], v);
          if constexpr (Agg::kCounts) atomicAdd(&counts[g[u]], 1ull);
        }
      }
    }
  };
  if (vvalid) rows(std::true_type{});
  else rows(std::false_type{});
  if constexpr (USE_LDS) {
    __syncthreads();
    for (int l = threadIdx.x; l < nl; l += kBlock) {
      const unsigned c = s_cnt[l];
      if (c) {
        agg.flush(s_w, l, (size_t)l);
        atomicAdd(&counts[l], (unsigned long long)c);
      }
    }
  }
}

// the grid of both regimes, and the launch: the LDS regime where the aggregate counts (WidenedAbsMax does not) and the groups fit
template <typename Agg, typename T>
int typed_agg(ah_ctx* c, const int32_t* ids, const T* vals, const uint8_t* vvalid, int64_t voff, int64_t n, void* counts, int64_t ngroups, Agg agg) {
  const bool lds = Agg::kCounts && ngroups <= kTypedLdsGroups;
  const int64_t steps = ah_ceil_div(n, (int64_t)kBlock * 8);
  const unsigned grid = lds ? ah_stream_grid(c, steps, /*default_bpc=*/2) : ah_stream_grid(c, steps);
  if constexpr (Agg::kCounts) {
    if (lds) typed_agg_kernel<Agg, T, true><<<grid, kBlock, 0, c->stream>>>(ids, vals, vvalid, voff, n, (unsigned long long*)counts, (int)ngroups, agg);
  }
  if (!lds) typed_agg_kernel<Agg, T, false><<<grid, kBlock, 0, c->stream>>>(ids, vals, vvalid, voff, n, (unsigned long long*)counts, (int)ngroups, agg);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

// ---- the second moment about the group's mean ----------------------------------------------------------------------
// The row's term is t = fl(d · d), d = fl(x − m_g), two separately rounded operations (the tree is built with -ffp-contract=off), x the
// value as a double: Float32 exactly, integers rounded to nearest even as the numeric cast rounds them (only 8-byte ones beyond 2^53 do).
__device__ __forceinline__ double sq_dev(unsigned long long bits, double mean) {
  const double d = __builtin_bit_cast(double, bits) - mean;
  return d * d;
}
// The policies of cast_agg_kernel.  Beside the members of the policies above: `Side`, the per-group words a row needs that are NOT its
// accumulators (ngroups words, cache-resident), and gather(g), which reads them; the kernel hands a row its own.
//
// The scale of a group's fixed-point sum: its largest finite non-zero term, as the bits of the double — the term being the value cast to
// Float64 (SQ false: the sum behind the mean) or its squared deviation (SQ true: M2).  Up to 4096 groups one LDS word per group, a look
// before the LDS atomic as in WidenedMinMax, the touched groups flushed once; above, WidenedAbsMax's shape: device atomics behind a
// look.  Nothing counted.  gmax: zeros at the start.
template <bool SQ>
struct GroupScale {
  static constexpr int kWords = 1;
  static constexpr bool kCounts = false;
  struct Side { double mean; };
  const double* means;   // SQ only
  unsigned long long* gmax;
  __device__ __forceinline__ Side gather(size_t g) const { return Side{SQ ? means[g] : 0.0}; }
  __device__ static __forceinline__ unsigned long long term(unsigned long long bits, Side s) {
    const unsigned long long a = (SQ ? __builtin_bit_cast(unsigned long long, sq_dev(bits, s.mean)) : bits) & ~kSignBit;
    return (a >> 52) == 0x7ff ? 0 : a;   // a non-finite term has no part in the scale
  }
  __device__ __forceinline__ void row_lds(unsigned long long* w, int l, size_t, unsigned long long bits, Side s) const {
    const unsigned long long a = term(bits, s);
    if (look_lds(&w[l]) < a) atomicMax(&w[l], a);
  }
  __device__ __forceinline__ void row_global(size_t g, unsigned long long bits, Side s) const {
    const unsigned long long a = term(bits, s);
    if (look(&gmax[g]) < a) atomicMax(&gmax[g], a);
  }
  __device__ __forceinline__ void flush(const unsigned long long* w, int l, size_t g) const {
    if (look(&gmax[g]) < w[l]) atomicMax(&gmax[g], w[l]);
  }
};
// Σ of the terms through the fixed-point accumulator at the group's own scale (fx.gmax is always set), a non-finite term to the flag
// words: WidenedSumFloat's accumulation with the scale — and for SQ the mean — handed in by the kernel.  SQ false: the term is the
// value cast to Float64 (the sum behind the mean); SQ true: its squared deviation (M2).  Counts the rows it adds.
template <bool SQ>
struct ScaledSum {
  static constexpr int kWords = 2;
  static constexpr bool kCounts = true;
  struct Side { double mean; unsigned long long scale; };
  FxAcc fx;
  const double* means;   // SQ only
  __device__ __forceinline__ Side gather(size_t g) const { return Side{SQ ? means[g] : 0.0, fx.gmax[g]}; }
  __device__ __forceinline__ void add(unsigned long long* lo_arr, unsigned long long* hi_arr, size_t slot, size_t g, unsigned long long bits, Side s) const {
    const double t = SQ ? sq_dev(bits, s.mean) : __builtin_bit_cast(double, bits);
    if (fx_finite(t)) {
      unsigned long long lo, hi;
      fx_split(t, fx_shift(s.scale), &lo, &hi);
      fx_add(lo_arr, hi_arr, slot, lo, hi);
    } else {
      atomicOr(&fx.flags[g], fx_flag(t));
    }
  }
  __device__ __forceinline__ void row_lds(unsigned long long* w, int l, size_t g, unsigned long long bits, Side s) const { add(w, w + kTypedLdsGroups, (size_t)l, g, bits, s); }
  __device__ __forceinline__ void row_global(size_t g, unsigned long long bits, Side s) const { add(fx.lo, fx.hi, g, g, bits, s); }
  __device__ __forceinline__ void flush(const unsigned long long* w, int l, size_t g) const { fx_add(fx.lo, fx.hi, g, w[l], w[kTypedLdsGroups + l]); }
};

// typed_agg_kernel's regimes, bounds check and loading rule (all loads of a step unconditional, from a row index clamped to n − 1, and
// issued before any value is used), for policies that read the column as cast to Float64.  The rule is extended to the gathers: the
// Side words of all eight rows go out in one go, behind the streaming loads and in front of the first row's use (an id that is not a
// group's gathers group 0, which exists, and the row is dropped as before) — gathered inside the row's branch, every row waited for its
// own gather before the next went out (measured).  The LDS regime always keeps its 32-bit row counts, to know the
// touched groups; they reach `counts` only for a policy that counts.  Zeros are the identity of every word.
template <typename Agg, typename T, bool USE_LDS>
__global__ __launch_bounds__(kBlock) void cast_agg_kernel(const int32_t* __restrict__ ids, const T* __restrict__ vals, const uint8_t* __restrict__ vvalid,
                                                           int64_t voff, int64_t n, unsigned long long* __restrict__ counts, int ngroups, Agg agg) {
  __shared__ unsigned long long s_w[USE_LDS ? Agg::kWords * kTypedLdsGroups : 1];
  __shared__ unsigned s_cnt[USE_LDS ? kTypedLdsGroups : 1];
  const int nl = USE_LDS && ngroups > kTypedLdsGroups ? kTypedLdsGroups : ngroups;
  if constexpr (USE_LDS) {
    for (int l = threadIdx.x; l < nl; l += kBlock) {
#pragma unroll
      for (int j = 0; j < Agg::kWords; j++) s_w[j * kTypedLdsGroups + l] = 0;
      s_cnt[l] = 0;
    }
    __syncthreads();
  }
  constexpr int U = 8;
  const int64_t stride = (int64_t)gridDim.x * kBlock * U;
  auto rows = [&](auto has_valid) {
    for (int64_t base = (int64_t)blockIdx.x * kBlock * U + threadIdx.x; base < n; base += stride) {
      int32_t g[U];
      T raw[U];
      uint8_t vb[U];
      typename Agg::Side side[U];
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int64_t i = base + (int64_t)u * kBlock, ic = i < n ? i : n - 1;
        g[u] = __builtin_nontemporal_load(&ids[ic]);
        raw[u] = __builtin_nontemporal_load(&vals[ic]);
        if constexpr (decltype(has_valid)::value) vb[u] = vvalid[(voff + ic) >> 3];
        else vb[u] = 0xff;
      }
#pragma unroll
      for (int u = 0; u < U; u++) side[u] = agg.gather((unsigned)g[u] < (unsigned)nl ? (size_t)g[u] : 0);
#pragma unroll
      for (int u = 0; u < U; u++) {
        const int64_t i = base + (int64_t)u * kBlock;
        const bool ok = i < n && ((vb[u] >> ((voff + i) & 7)) & 1);
        if (!ok || (unsigned)g[u] >= (unsigned)nl) continue;
        const unsigned long long v = __builtin_bit_cast(unsigned long long, (double)raw[u]);
        if constexpr (USE_LDS) {
          agg.row_lds(s_w, g[u], (size_t)g[u], v, side[u]);
          atomicAdd(&s_cnt[g[u]], 1u);
        } else {
          agg.row_global((size_t)g[u], v, side[u]);
          if constexpr (Agg::kCounts) atomicAdd(&counts[g[u]], 1ull);
        }
      }
    }
  };
  if (vvalid) rows(std::true_type{});
  else rows(std::false_type{});
  if constexpr (USE_LDS) {
    __syncthreads();
    for (int l = threadIdx.x; l < nl; l += kBlock) {
      const unsigned c = s_cnt[l];
      if (c) {
        agg.flush(s_w, l, (size_t)l);
        if constexpr (Agg::kCounts) atomicAdd(&counts[l], (unsigned long long)c);
      }
    }
  }
}

// its launch: one regime per call, so only kernels that can run are built.  `counts` is read by a policy that counts only.
template <typename T, typename Agg>
int cast_agg(ah_ctx* c, const int32_t* ids, const T* vals, const uint8_t* vvalid, int64_t voff, int64_t n, void* counts, int64_t ngroups, Agg agg) {
  const int64_t steps = ah_ceil_div(n, (int64_t)kBlock * 8);
  if (ngroups <= kTypedLdsGroups)
    cast_agg_kernel<Agg, T, true><<<ah_stream_grid(c, steps, /*default_bpc=*/2), kBlock, 0, c->stream>>>(ids, vals, vvalid, voff, n, (unsigned long long*)counts, (int)ngroups, agg);
  else
    cast_agg_kernel<Agg, T, false><<<ah_stream_grid(c, steps), kBlock, 0, c->stream>>>(ids, vals, vvalid, voff, n, (unsigned long long*)counts, (int)ngroups, agg);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

// out[0] = bits of the largest finite |x| of the Float32 column as a double, out[1] = largest fx_inv_exp of its non-zero finite values
// as doubles (the range words of ah_hashing.h's absmax_kernel, which reads doubles); both zeroed by the caller.  Streams like that
// kernel: 16 bytes per lane and load (four values, element-aligned), four loads in flight, converted after the loads have gone out; a
// grid-stride loop over ≈ 2 workgroups per CU; one atomic pair per workgroup.
__global__ __launch_bounds__(kBlock) void typed_absmax_kernel(const float* __restrict__ vals, const uint8_t* __restrict__ vvalid, int64_t voff, int64_t n,
                                                               unsigned long long* __restrict__ out) {
  unsigned long long m = 0;
  unsigned im = 0;
  constexpr int U = 4;
  const int64_t nvec = n >> 2;
  // one value: a finite non-zero |x| inside the current [min exponent, max] changes nothing and skips the validity read
  auto one = [&](float x, int64_t i) {
    const unsigned long long b = widen<float>(x) & ~kSignBit;
    if ((b >> 52) != 0x7ff && b != 0 && (b > m || fx_inv_exp(b) > im) && ah_bit(vvalid, voff + i)) {
      m = b > m ? b : m;
      im = fx_inv_exp(b) > im ? fx_inv_exp(b) : im;
    }
  };
  const int64_t stride = (int64_t)gridDim.x * kBlock * U;
  for (int64_t base = (int64_t)blockIdx.x * kBlock * U + threadIdx.x; base < nvec; base += stride) {
    ah_vec16<float> x[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t j = base + (int64_t)u * kBlock;
      if (j < nvec) x[u] = ah_ld16_nt<float>(vals + 4 * j);
      else { x[u].v[0] = x[u].v[1] = x[u].v[2] = x[u].v[3] = 0.0f; }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t j = base + (int64_t)u * kBlock;
#pragma unroll
      for (int k = 0; k < 4; k++) one(x[u].v[k], 4 * j + k);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int64_t i = nvec << 2; i < n; i++) one(vals[i], i);
  ah_wave_max2(m, im);
  __shared__ unsigned long long s_m[kBlock / 64];
  __shared__ unsigned s_im[kBlock / 64];
  if ((threadIdx.x & 63) == 0) { s_m[threadIdx.x >> 6] = m; s_im[threadIdx.x >> 6] = im; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kBlock / 64; w++) { m = s_m[w] > m ? s_m[w] : m; im = s_im[w] > im ? s_im[w] : im; }
    if (m) atomicMax(&out[0], m);
    if (im) atomicMax(&out[1], (unsigned long long)im);
  }
}

__global__ __launch_bounds__(kBlock) void typed_min_max_init_kernel(unsigned long long* __restrict__ mins, unsigned long long* __restrict__ maxs,
                                                                     unsigned long long* __restrict__ counts, int64_t ngroups) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g < ngroups) { mins[g] = kMinIdentity; maxs[g] = kMaxIdentity; counts[g] = 0; }
}

// ordered 64-bit words → values of the input type: zeros for a group without valid values, the canonical quiet NaN for a group of NaNs
template <typename T>
__global__ __launch_bounds__(kBlock) void typed_min_max_finish_kernel(const unsigned long long* __restrict__ mins, const unsigned long long* __restrict__ maxs,
                                                                       const unsigned long long* __restrict__ counts, int64_t ngroups,
                                                                       T* __restrict__ out_mins, T* __restrict__ out_maxs) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= ngroups) return;
  constexpr int KIND = kind_of<T>();
  const unsigned long long lo = mins[g], hi = maxs[g];
  T omin, omax;
  if (counts[g] == 0) {
    omin = omax = T(0);
  } else if (KIND == kF64 && lo == kMinIdentity) {
    if constexpr (std::is_same<T, float>::value) omin = omax = __builtin_bit_cast(float, kQuietNaN32);
    else omin = omax = T(0);
  } else if constexpr (std::is_same<T, float>::value) {
    omin = (float)__builtin_bit_cast(double, from_ordered<KIND>(lo));   // exact: the double came from a float
    omax = (float)__builtin_bit_cast(double, from_ordered<KIND>(hi));
  } else {
    omin = (T)from_ordered<KIND>(lo);   // the low bytes of a value that was widened from T
    omax = (T)from_ordered<KIND>(hi);
  }
  out_mins[g] = omin;
  out_maxs[g] = omax;
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void group_mean_kernel(const unsigned long long* __restrict__ sums, const long long* __restrict__ counts, int64_t ngroups,
                                                             double* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= ngroups) return;
  const long long c = counts[g];
  const unsigned long long s = sums[g];
  double x;
  if constexpr (KIND == kU64) x = (double)s;
  else if constexpr (KIND == kI64) x = (double)(long long)s;
  else x = __builtin_bit_cast(double, s);
  out[g] = c ? x / (double)c : 0.0;
}

// out[g] = m2[g] / (double)(counts[g] − ddof), or its correctly rounded square root; 0.0 where counts[g] ≤ ddof
__global__ __launch_bounds__(kBlock) void group_variance_kernel(const double* __restrict__ m2, const long long* __restrict__ counts, int64_t ngroups,
                                                                 long long ddof, bool take_sqrt, double* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= ngroups) return;
  const long long c = counts[g];
  double v = 0.0;
  if (c > ddof) {
    v = m2[g] / (double)(c - ddof);
    if (take_sqrt) v = __dsqrt_rn(v);
  }
  out[g] = v;
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
int typed_check(ah_ctx* c, const char* who, int64_t ngroups, int64_t voff, int64_t n, bool buffers, bool* nothing) {
  *nothing = true;
  if (n < 0 || voff < 0 || ngroups < 0) return ah_fail(c, AH_EINVALID, "%s: negative length/offset", who);
  if (ngroups > 0x7fffffffll) return ah_fail(c, AH_EINVALID, "%s: more than 2^31 - 1 groups", who);
  if (n > ((int64_t)1 << 30)) return ah_fail(c, AH_ENOTIMPL, "%s: more than 2^30 rows per call", who);
  if (ngroups == 0) return AH_OK;
  if (!buffers) return ah_fail(c, AH_EINVALID, "%s: null buffer", who);
  *nothing = false;
  return AH_OK;
}

template <typename T>
int sum_int_typed(ah_ctx* c, const int32_t* ids, int64_t ng, const T* vals, const uint8_t* vvalid, int64_t voff, int64_t n, void* out_sums, int64_t* out_counts) {
  AH_HIP(c, hipMemsetAsync(out_sums, 0, (size_t)ng * 8, c->stream));
  AH_HIP(c, hipMemsetAsync(out_counts, 0, (size_t)ng * sizeof(int64_t), c->stream));
  return typed_agg(c, ids, vals, vvalid, voff, n, out_counts, ng, WidenedSumInt{(unsigned long long*)out_sums});
}

int sum_f32(ah_ctx* c, const int32_t* ids, int64_t ng, const float* vals, const uint8_t* vvalid, int64_t voff, int64_t n, double* out_sums, int64_t* out_counts) {
  // temporaries: 128-bit accumulators and a flag word per group, the call's range words, a scale per group for a wide column
  TempCarver t;
  unsigned long long *lo, *hi, *range, *gmax;
  unsigned* flags;
  auto carve = [&](TempCarver& k) { k.take(lo, (size_t)ng); k.take(hi, (size_t)ng); k.take(flags, (size_t)ng); k.take(range, 2); k.take(gmax, (size_t)ng); };
  carve(t);
  void* arena = nullptr;
  int rc = ah_temp_reserve(c, t.used, &arena);
  if (rc != AH_OK) return rc;
  t = TempCarver{(uint8_t*)arena, 0};
  carve(t);
  AH_HIP(c, hipMemsetAsync(range, 0, 16, c->stream));
  typed_absmax_kernel<<<ah_stream_grid(c, ah_ceil_div(n, (int64_t)kBlock * 16), 2), kBlock, 0, c->stream>>>(vals, vvalid, voff, n, range);
  AH_LAUNCH_CHECK(c);
  AH_HIP(c, hipMemsetAsync(out_counts, 0, (size_t)ng * sizeof(int64_t), c->stream));
  AH_HIP(c, hipMemsetAsync(lo, 0, (size_t)ng * 8, c->stream));
  AH_HIP(c, hipMemsetAsync(hi, 0, (size_t)ng * 8, c->stream));
  AH_HIP(c, hipMemsetAsync(flags, 0, (size_t)ng * 4, c->stream));
  // one scale for the call, or one per group?  (ah_hashing.h: a column spanning more than 42 binades)
  AH_HIP(c, hipMemcpyAsync(&c->pinned[2], range, 16, hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipStreamSynchronize(c->stream));
  FxAcc fx{lo, hi, flags, range, nullptr};
  if (fx_wide(*(volatile uint64_t*)&c->pinned[2], *(volatile uint64_t*)&c->pinned[3])) {
    AH_HIP(c, hipMemsetAsync(gmax, 0, (size_t)ng * 8, c->stream));
    if ((rc = typed_agg(c, ids, vals, vvalid, voff, n, nullptr, ng, WidenedAbsMax{gmax})) != AH_OK) return rc;
    fx.gmax = gmax;
  }
  if ((rc = typed_agg(c, ids, vals, vvalid, voff, n, out_counts, ng, WidenedSumFloat{fx, 0})) != AH_OK) return rc;
  fx_finalize_kernel<<<(unsigned)ah_ceil_div(ng, kBlock), kBlock, 0, c->stream>>>(fx, ng, out_sums);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

template <typename T>
int min_max_typed(ah_ctx* c, const int32_t* ids, int64_t ng, const T* vals, const uint8_t* vvalid, int64_t voff, int64_t n, void* out_mins, void* out_maxs,
                  int64_t* out_counts) {
  void* arena = nullptr;
  int rc = ah_temp_reserve(c, 2 * ah_pad((size_t)ng * 8), &arena);
  if (rc != AH_OK) return rc;
  unsigned long long *mins = (unsigned long long*)arena, *maxs = (unsigned long long*)((uint8_t*)arena + ah_pad((size_t)ng * 8));
  unsigned long long* counts = (unsigned long long*)out_counts;
  const unsigned gblocks = (unsigned)ah_ceil_div(ng, kBlock);
  typed_min_max_init_kernel<<<gblocks, kBlock, 0, c->stream>>>(mins, maxs, counts, ng);
  AH_LAUNCH_CHECK(c);
  if (n > 0 && (rc = typed_agg(c, ids, vals, vvalid, voff, n, counts, ng, WidenedMinMax<kind_of<T>()>{mins, maxs})) != AH_OK) return rc;
  typed_min_max_finish_kernel<T><<<gblocks, kBlock, 0, c->stream>>>(mins, maxs, counts, ng, (T*)out_mins, (T*)out_maxs);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

// the temporaries of ah_group_m2, ngroups entries each: the 128-bit accumulators, the scales, the counts of the M2 pass, the flag words
struct FxTemps { unsigned long long *lo, *hi, *gmax, *cnt; unsigned* flags; };
int fx_temps(ah_ctx* c, int64_t ng, FxTemps* t) {
  auto carve = [&](TempCarver& k) { k.take(t->lo, (size_t)ng); k.take(t->hi, (size_t)ng); k.take(t->gmax, (size_t)ng); k.take(t->cnt, (size_t)ng); k.take(t->flags, (size_t)ng); };
  TempCarver k;
  carve(k);
  void* arena = nullptr;
  int rc = ah_temp_reserve(c, k.used, &arena);
  if (rc != AH_OK) return rc;
  k = TempCarver{(uint8_t*)arena, 0};
  carve(k);
  return AH_OK;
}
int fx_temps_clear(ah_ctx* c, int64_t ng, const FxTemps& t) {
  AH_HIP(c, hipMemsetAsync(t.lo, 0, (size_t)ng * 8, c->stream));
  AH_HIP(c, hipMemsetAsync(t.hi, 0, (size_t)ng * 8, c->stream));
  AH_HIP(c, hipMemsetAsync(t.gmax, 0, (size_t)ng * 8, c->stream));
  AH_HIP(c, hipMemsetAsync(t.cnt, 0, (size_t)ng * 8, c->stream));
  AH_HIP(c, hipMemsetAsync(t.flags, 0, (size_t)ng * 4, c->stream));
  return AH_OK;
}
// The reproducible Float64 group sums of a column of ANY numeric type read as cast to Float64, and the counts: always at the group's
// own scale.  THE BYTES are those of ah_group_sum_f64 on the cast column: where that call takes one scale (a column spanning ≤ 42
// binades) no addend is truncated at either scale, so both 128-bit sums are exact and round to the same double; where it takes a
// scale per group it is this one.  Two passes over the column.  The temporaries are the caller's.
template <typename T>
int sum_cast_f64(ah_ctx* c, const int32_t* ids, int64_t ng, const T* vals, const uint8_t* vvalid, int64_t voff, int64_t n, const FxTemps& t,
                 double* out_sums, int64_t* out_counts) {
  int rc;
  if ((rc = fx_temps_clear(c, ng, t)) != AH_OK) return rc;
  AH_HIP(c, hipMemsetAsync(out_counts, 0, (size_t)ng * sizeof(int64_t), c->stream));
  if ((rc = cast_agg(c, ids, vals, vvalid, voff, n, nullptr, ng, GroupScale<false>{nullptr, t.gmax})) != AH_OK) return rc;
  const FxAcc fx{t.lo, t.hi, t.flags, nullptr, t.gmax};
  if ((rc = cast_agg(c, ids, vals, vvalid, voff, n, out_counts, ng, ScaledSum<false>{fx, nullptr})) != AH_OK) return rc;
  fx_finalize_kernel<<<(unsigned)ah_ceil_div(ng, kBlock), kBlock, 0, c->stream>>>(fx, ng, out_sums);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

// means, M2 and counts of one column.  Passes over the column: the sum (one for an integer narrower than 8 bytes, whose exact wrapping
// sum cannot wrap below 2^30 rows and converts once to the same double; two for every other type), the scale (the largest finite t per
// group) and the accumulation of the t: three or four.  Nothing per row goes to HBM; out_m2 holds the sums until the means are taken.
template <typename T>
int m2_typed(ah_ctx* c, const int32_t* ids, int64_t ng, const T* vals, const uint8_t* vvalid, int64_t voff, int64_t n, double* out_means, double* out_m2,
             int64_t* out_counts) {
  int rc;
  const unsigned gblocks = (unsigned)ah_ceil_div(ng, kBlock);
  constexpr bool kIntSum = std::is_integral<T>::value && sizeof(T) < 8;
  if constexpr (kIntSum) {   // (the temporaries are reserved behind it: the reservation may move the arena)
    if ((rc = sum_int_typed<T>(c, ids, ng, vals, vvalid, voff, n, out_m2, out_counts)) != AH_OK) return rc;
    group_mean_kernel<kind_of<T>()><<<gblocks, kBlock, 0, c->stream>>>((const unsigned long long*)out_m2, (const long long*)out_counts, ng, out_means);
    AH_LAUNCH_CHECK(c);
  }
  FxTemps t;
  if ((rc = fx_temps(c, ng, &t)) != AH_OK) return rc;
  if constexpr (!kIntSum) {
    if ((rc = sum_cast_f64<T>(c, ids, ng, vals, vvalid, voff, n, t, out_m2, out_counts)) != AH_OK) return rc;
    group_mean_kernel<kF64><<<gblocks, kBlock, 0, c->stream>>>((const unsigned long long*)out_m2, (const long long*)out_counts, ng, out_means);
    AH_LAUNCH_CHECK(c);
  }
  if ((rc = fx_temps_clear(c, ng, t)) != AH_OK) return rc;
  if ((rc = cast_agg(c, ids, vals, vvalid, voff, n, nullptr, ng, GroupScale<true>{out_means, t.gmax})) != AH_OK) return rc;
  const FxAcc fx{t.lo, t.hi, t.flags, nullptr, t.gmax};
  // (the kernel counts what it accumulates; the counts of the sum stand, these go to a temporary)
  if ((rc = cast_agg(c, ids, vals, vvalid, voff, n, t.cnt, ng, ScaledSum<true>{fx, out_means})) != AH_OK) return rc;
  fx_finalize_kernel<<<gblocks, kBlock, 0, c->stream>>>(fx, ng, out_m2);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

// the narrow types: every numeric type but the three 8-byte ones, which forward
template <class F>
bool with_narrow_type(int type, F&& f) {
  return ah_type_width(type) < 8 && with_numeric_type(type, [&](auto t) {
    using T = typename decltype(t)::type;
    if constexpr (sizeof(T) < 8) f(t);
  });
}

}  // namespace

AH_EXPORT int ah_group_count(ah_ctx* c, const int32_t* ids, int64_t ngroups, const uint8_t* vvalid, int64_t voff, int64_t n, int64_t* out_counts) {
  AH_ENTER(c);
  bool nothing;
  int rc = typed_check(c, "group_count", ngroups, voff, n, out_counts && (n == 0 || ids), &nothing);
  if (rc != AH_OK || nothing) return rc;
  AH_HIP(c, hipMemsetAsync(out_counts, 0, (size_t)ngroups * sizeof(int64_t), c->stream));
  if (n == 0) return AH_OK;
  return typed_agg(c, ids, (const uint8_t*)nullptr, vvalid, voff, n, out_counts, ngroups, CountRows{});
}

AH_EXPORT int ah_group_sum_typed(ah_ctx* c, int type, const int32_t* ids, int64_t ngroups, const void* vals, const uint8_t* vvalid, int64_t voff,
                                 int64_t n, void* out_sums, int64_t* out_counts) {
  AH_ENTER(c);
  if (!ah_type_width(type)) return ah_fail(c, AH_ENOTIMPL, "group_sum_typed: type id %d is not a numeric type", type);
  if (type == AH_FLOAT64) return ah_group_sum_f64(c, ids, ngroups, (const double*)vals, vvalid, voff, n, (double*)out_sums, out_counts);
  if (type == AH_INT64 || type == AH_UINT64)   // a wrapping 64-bit sum has one bit pattern, signed or not
    return ah_group_sum_i64(c, ids, ngroups, (const int64_t*)vals, vvalid, voff, n, (int64_t*)out_sums, out_counts);
  bool nothing;
  int rc = typed_check(c, "group_sum_typed", ngroups, voff, n, out_sums && out_counts && (n == 0 || (ids && vals)), &nothing);
  if (rc != AH_OK || nothing) return rc;
  if (n == 0) {   // no rows: every group is empty
    AH_HIP(c, hipMemsetAsync(out_sums, 0, (size_t)ngroups * 8, c->stream));
    AH_HIP(c, hipMemsetAsync(out_counts, 0, (size_t)ngroups * sizeof(int64_t), c->stream));
    return AH_OK;
  }
  with_narrow_type(type, [&](auto t) {
    using T = typename decltype(t)::type;
    if constexpr (std::is_same<T, float>::value) rc = sum_f32(c, ids, ngroups, (const float*)vals, vvalid, voff, n, (double*)out_sums, out_counts);
    else rc = sum_int_typed<T>(c, ids, ngroups, (const T*)vals, vvalid, voff, n, out_sums, out_counts);
  });
  return rc;
}

AH_EXPORT int ah_group_min_max_typed(ah_ctx* c, int type, const int32_t* ids, int64_t ngroups, const void* vals, const uint8_t* vvalid,
                                     int64_t voff, int64_t n, void* out_mins, void* out_maxs, int64_t* out_counts) {
  AH_ENTER(c);
  if (!ah_type_width(type)) return ah_fail(c, AH_ENOTIMPL, "group_min_max_typed: type id %d is not a numeric type", type);
  if (type == AH_FLOAT64)
    return ah_group_min_max_f64(c, ids, ngroups, (const double*)vals, vvalid, voff, n, (double*)out_mins, (double*)out_maxs, out_counts);
  if (type == AH_INT64)
    return ah_group_min_max_i64(c, ids, ngroups, (const int64_t*)vals, vvalid, voff, n, (int64_t*)out_mins, (int64_t*)out_maxs, out_counts);
  if (type == AH_UINT64)
    return ah_group_min_max_u64(c, ids, ngroups, (const uint64_t*)vals, vvalid, voff, n, (uint64_t*)out_mins, (uint64_t*)out_maxs, out_counts);
  bool nothing;
  int rc = typed_check(c, "group_min_max_typed", ngroups, voff, n, out_mins && out_maxs && out_counts && (n == 0 || (ids && vals)), &nothing);
  if (rc != AH_OK || nothing) return rc;
  with_narrow_type(type, [&](auto t) {
    using T = typename decltype(t)::type;
    rc = min_max_typed<T>(c, ids, ngroups, (const T*)vals, vvalid, voff, n, out_mins, out_maxs, out_counts);
  });
  return rc;
}

AH_EXPORT int ah_group_mean(ah_ctx* c, int sum_type, const void* sums, const int64_t* counts, int64_t ngroups, double* out_means) {
  AH_ENTER(c);
  if (ngroups < 0) return ah_fail(c, AH_EINVALID, "group_mean: negative length/offset");
  if (sum_type != AH_INT64 && sum_type != AH_UINT64 && sum_type != AH_FLOAT64)
    return ah_fail(c, AH_ENOTIMPL, "group_mean: sums are Int64, UInt64 or Float64, not type id %d", sum_type);
  if (ngroups == 0) return AH_OK;
  if (!sums || !counts || !out_means) return ah_fail(c, AH_EINVALID, "group_mean: null buffer");
  const unsigned grid = (unsigned)ah_ceil_div(ngroups, kBlock);
  const unsigned long long* s = (const unsigned long long*)sums;
  const long long* n = (const long long*)counts;
  if (sum_type == AH_INT64) group_mean_kernel<kI64><<<grid, kBlock, 0, c->stream>>>(s, n, ngroups, out_means);
  else if (sum_type == AH_UINT64) group_mean_kernel<kU64><<<grid, kBlock, 0, c->stream>>>(s, n, ngroups, out_means);
  else group_mean_kernel<kF64><<<grid, kBlock, 0, c->stream>>>(s, n, ngroups, out_means);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

AH_EXPORT int ah_group_m2(ah_ctx* c, int type, const int32_t* ids, int64_t ngroups, const void* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                          double* out_means, double* out_m2, int64_t* out_counts) {
  AH_ENTER(c);
  if (!ah_type_width(type)) return ah_fail(c, AH_ENOTIMPL, "group_m2: type id %d is not a numeric type", type);
  bool nothing;
  int rc = typed_check(c, "group_m2", ngroups, voff, n, out_means && out_m2 && out_counts && (n == 0 || (ids && vals)), &nothing);
  if (rc != AH_OK || nothing) return rc;
  if (n == 0) {   // no rows: every group is empty
    AH_HIP(c, hipMemsetAsync(out_means, 0, (size_t)ngroups * 8, c->stream));
    AH_HIP(c, hipMemsetAsync(out_m2, 0, (size_t)ngroups * 8, c->stream));
    AH_HIP(c, hipMemsetAsync(out_counts, 0, (size_t)ngroups * sizeof(int64_t), c->stream));
    return AH_OK;
  }
  with_numeric_type(type, [&](auto t) {
    using T = typename decltype(t)::type;
    rc = m2_typed<T>(c, ids, ngroups, (const T*)vals, vvalid, voff, n, out_means, out_m2, out_counts);
  });
  return rc;
}

AH_EXPORT int ah_group_variance(ah_ctx* c, const double* m2, const int64_t* counts, int64_t ngroups, int ddof, int take_sqrt, double* out) {
  AH_ENTER(c);
  if (ngroups < 0) return ah_fail(c, AH_EINVALID, "group_variance: negative length/offset");
  if (ddof < 0) return ah_fail(c, AH_EINVALID, "group_variance: negative ddof (%d)", ddof);
  if (ngroups == 0) return AH_OK;
  if (!m2 || !counts || !out) return ah_fail(c, AH_EINVALID, "group_variance: null buffer");
  group_variance_kernel<<<(unsigned)ah_ceil_div(ngroups, kBlock), kBlock, 0, c->stream>>>(m2, (const long long*)counts, ngroups, (long long)ddof,
                                                                                          take_sqrt != 0, out);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}
