// ah_hash_agg.hip — the aggregates over dense group ids: group-by sum (ah_hash_sum_*) and group-by min / max (ah_hash_min_max_*).
//
// No reference analogue (arrow-go has no hash aggregate); definitions in DESIGN.md §3.2.  The ids are dictionary_encode's (ah_hash.hip,
// reached through ah_encode_u64_groups): dense, in first-seen order.  This path answers every call the partition-first group-by
// (ah_groupby.hip) declines.
//
// ONE kernel skeleton, group_agg_kernel<Agg, USE_LDS>, walks the rows; an aggregate is a policy — what a group's LDS words start as, how
// one row's value enters an LDS slot or the global accumulators, how a touched LDS slot is flushed:
//   SumI64      wrapping 64-bit sum                                           (LDS: sum)
//   SumF64      128-bit fixed-point sum (ah_hashing.h), rounded once          (LDS: low word, high word)
//   MinMax<K>   atomicMin / atomicMax on order-preserving words, behind a look  (LDS: min, max)
//   AbsMax      largest finite |x| per group, the scale of a wide Float64 sum (global only)
// The skeleton counts the rows of a group itself (LDS: one 32-bit count per group, which also says "touched").
//
// Regimes, by the number of groups:
//   ≤ 4096   every workgroup keeps all groups in LDS (12 or 20 B per group, two workgroups per CU): rows hit LDS atomics, each
//            workgroup flushes every touched group to HBM once — instead of same-address device atomics per row (~12 ns each,
//            serialised at L2).
//   > 4096   sums: the (value, id) pairs are partitioned by id >> 12 first and bucket_sum_kernel aggregates run by run in LDS (below);
//            min / max, wide Float64 sums and option hash_sum_partition = 0: device atomics straight into the accumulators.
// HBM: 12 B/row (id + value) + the validity bits.
#include "ah_common.h"
#include "ah_hashing.h"
#include "ah_group_order.h"

namespace {

constexpr int kLdsGroups = 4096;

// ---- the policies ------------------------------------------------------------------------------------------------------------------
// kWords 64-bit LDS words per group (word j of slot l is w[j · kLdsGroups + l]), identity(j) what they start as; begin() once per
// thread; row_lds(w, l, g, bits): a valid row of global group g into LDS slot l; row_global(g, bits): the same into the global
// accumulators; flush(w, l, g): slot l into the global accumulators of group g.  kCounts: the skeleton counts the rows.
struct SumI64 {
  static constexpr int kWords = 1;
  static constexpr bool kCounts = true;
  unsigned long long* sums;
  __device__ static constexpr unsigned long long identity(int) { return 0; }
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void row_lds(unsigned long long* w, int l, size_t, unsigned long long bits) const { atomicAdd(&w[l], bits); }
  __device__ __forceinline__ void row_global(size_t g, unsigned long long bits) const { atomicAdd(&sums[g], bits); }
  __device__ __forceinline__ void flush(const unsigned long long* w, int l, size_t g) const { atomicAdd(&sums[g], w[l]); }
};

struct SumF64 {   // fx.gmax set (wide columns): the group's own scale, looked up per row
  static constexpr int kWords = 2;
  static constexpr bool kCounts = true;
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
  __device__ __forceinline__ void row_lds(unsigned long long* w, int l, size_t g, unsigned long long bits) const { add(w, w + kLdsGroups, (size_t)l, g, bits); }
  __device__ __forceinline__ void row_global(size_t g, unsigned long long bits) const { add(fx.lo, fx.hi, g, g, bits); }
  __device__ __forceinline__ void flush(const unsigned long long* w, int l, size_t g) const { fx_add(fx.lo, fx.hi, g, w[l], w[kLdsGroups + l]); }
};

template <int KIND>
struct MinMax {   // mins / maxs hold the identities, the counts zeros, for all groups when the aggregate starts
  static constexpr int kWords = 2;
  static constexpr bool kCounts = true;
  unsigned long long *mins, *maxs;
  __device__ static constexpr unsigned long long identity(int j) { return j == 0 ? kMinIdentity : kMaxIdentity; }
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void row_lds(unsigned long long* w, int l, size_t, unsigned long long bits) const {
    if (is_nan_bits<KIND>(bits)) return;
    const unsigned long long x = to_ordered<KIND>(bits);
    if (x < look_lds(&w[l])) atomicMin(&w[l], x);
    if (x > look_lds(&w[kLdsGroups + l])) atomicMax(&w[kLdsGroups + l], x);
  }
  __device__ __forceinline__ void row_global(size_t g, unsigned long long bits) const {
    if (is_nan_bits<KIND>(bits)) return;
    const unsigned long long x = to_ordered<KIND>(bits);
    if (x < look(&mins[g])) atomicMin(&mins[g], x);
    if (x > look(&maxs[g])) atomicMax(&maxs[g], x);
  }
  __device__ __forceinline__ void flush(const unsigned long long* w, int l, size_t g) const {
    const unsigned long long lo = w[l], hi = w[kLdsGroups + l];
    if (lo < look(&mins[g])) atomicMin(&mins[g], lo);
    if (hi > look(&maxs[g])) atomicMax(&maxs[g], hi);
  }
};

// wide columns (ah_hashing.h): largest finite |x| per group = the group's fixed-point scale.  A look before the atomic: once a
// group's maximum has been seen (early, on average) its rows issue none.  Global only: no LDS words, nothing counted.
struct AbsMax {
  static constexpr int kWords = 0;
  static constexpr bool kCounts = false;
  unsigned long long* gmax;   // zeros when the aggregate starts
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void row_global(size_t g, unsigned long long bits) const {
    const unsigned long long a = bits & ~kSignBit;
    if ((a >> 52) == 0x7ff || a == 0) return;
    if (look(&gmax[g]) < a) atomicMax(&gmax[g], a);
  }
};

// ---- the skeleton ------------------------------------------------------------------------------------------------------------------
// the pieces bucket_sum_kernel shares with it: fill the first nl LDS slots, one row, flush the touched ones among the first nl slots
// into the groups base + slot
template <typename Agg>
__device__ __forceinline__ void lds_fill(unsigned long long* w, unsigned* cnt, int nl) {
  for (int l = threadIdx.x; l < nl; l += kBlock) {
#pragma unroll
    for (int j = 0; j < Agg::kWords; j++) w[j * kLdsGroups + l] = Agg::identity(j);
    cnt[l] = 0;
  }
  __syncthreads();
}
template <typename Agg>
__device__ __forceinline__ void lds_row(const Agg& agg, unsigned long long* w, unsigned* cnt, int l, size_t g, unsigned long long bits) {
  agg.row_lds(w, l, g, bits);
  atomicAdd(&cnt[l], 1u);
}
template <typename Agg>
__device__ __forceinline__ void global_row(const Agg& agg, unsigned long long* counts, size_t g, unsigned long long bits) {
  agg.row_global(g, bits);
  if constexpr (Agg::kCounts) atomicAdd(&counts[g], 1ull);
}
template <typename Agg>
__device__ __forceinline__ void lds_flush(const Agg& agg, const unsigned long long* w, const unsigned* cnt, int nl, unsigned long long* counts, size_t base) {
  __syncthreads();
  for (int l = threadIdx.x; l < nl; l += kBlock) {
    const unsigned n = cnt[l];
    if (n) {
      agg.flush(w, l, base + l);
      atomicAdd(&counts[base + l], (unsigned long long)n);
    }
  }
}

// USE_LDS: ngroups ≤ kLdsGroups (the host's choice).  An id outside [0, ngroups) — there is none among encode's — touches nothing.
template <typename Agg, bool USE_LDS>
__global__ __launch_bounds__(kBlock) void group_agg_kernel(const int32_t* __restrict__ ids, const unsigned long long* __restrict__ vals,
                                                            const uint8_t* __restrict__ vvalid, int64_t voff, int64_t n,
                                                            unsigned long long* __restrict__ counts, int ngroups, Agg agg) {
  __shared__ unsigned long long s_w[USE_LDS ? Agg::kWords * kLdsGroups : 1];
  __shared__ unsigned s_cnt[USE_LDS ? kLdsGroups : 1];
  const int nl = USE_LDS && ngroups > kLdsGroups ? kLdsGroups : ngroups;
  if constexpr (USE_LDS) lds_fill<Agg>(s_w, s_cnt, nl);
  agg.begin();
  constexpr int U = 8;  // rows per lane per step: 8 id loads + 8 value loads in flight (one row at a time is latency-bound)
  const int64_t stride = (int64_t)gridDim.x * kBlock * U;
  for (int64_t base = (int64_t)blockIdx.x * kBlock * U + threadIdx.x; base < n; base += stride) {
    int32_t g[U];
    unsigned long long v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = base + (int64_t)u * kBlock;
      const bool ok = i < n && ah_bit(vvalid, voff + i);
      g[u] = ok ? __builtin_nontemporal_load(&ids[i]) : -1;
      v[u] = ok ? __builtin_nontemporal_load(&vals[i]) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      if ((unsigned)g[u] >= (unsigned)nl) continue;   // a null value (−1), or an id that is not a group's: out of memory it does not own
      if constexpr (USE_LDS) lds_row(agg, s_w, s_cnt, g[u], (size_t)g[u], v[u]);
      else global_row(agg, counts, (size_t)g[u], v[u]);
    }
  }
  if constexpr (USE_LDS) lds_flush(agg, s_w, s_cnt, nl, counts, 0);
}

// the grid of both regimes, and the launch: the LDS regime where the aggregate has LDS words and the groups fit
template <typename Agg>
int group_agg(ah_ctx* c, const int32_t* ids, const void* vals, const uint8_t* vvalid, int64_t voff, int64_t n, void* counts, int64_t ngroups, Agg agg) {
  const bool lds = Agg::kWords > 0 && ngroups <= kLdsGroups;
  const unsigned grid = lds ? ah_stream_grid(c, ah_ceil_div(n, (int64_t)kBlock * 8), /*default_bpc=*/2) : ah_stream_grid(c, ah_ceil_div(n, (int64_t)kBlock * 8));
  const int ng = (int)(ngroups > 0x7fffffff ? 0x7fffffff : ngroups);
  if constexpr (Agg::kWords > 0) {
    if (lds) group_agg_kernel<Agg, true><<<grid, kBlock, 0, c->stream>>>(ids, (const unsigned long long*)vals, vvalid, voff, n, (unsigned long long*)counts, ng, agg);
  }
  if (!lds) group_agg_kernel<Agg, false><<<grid, kBlock, 0, c->stream>>>(ids, (const unsigned long long*)vals, vvalid, voff, n, (unsigned long long*)counts, ng, agg);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

// Above 4 Ki groups LDS cannot hold all groups, and two global atomics per row run at ≈ 25 G atomics/s
// device-wide (5.4 ms for 2^26 rows, whatever the number of copies of the sums — measured).  So the
// (value, group id) pairs are first partitioned by id >> 12 with ah_sort.hip's stable radix kernels — one
// 256-way pass up to 1 Mi groups, two passes (65 536 windows) up to 256 Mi — which makes every 64 Ki-row
// chunk a short sequence of runs, each inside one 4096-group window.  A workgroup walks the runs of its
// chunk: aggregate the run in LDS, flush the groups it touched (consecutive addresses), next run.
constexpr int kBucketShift = 12;                     // log2(kLdsGroups)
constexpr int64_t kPartitionOnePass = 1 << 20;       // 256 windows of 4096 groups
constexpr int64_t kPartitionMaxGroups = 1ll << 28;   // 65 536 windows
constexpr int64_t kChunkRows = 1 << 16;
constexpr int64_t kShortRun = 1024;                  // runs shorter than this go straight to global atomics

template <typename Agg>   // SumI64 or SumF64 with the call's one scale (a wide column does not come here)
__global__ __launch_bounds__(kBlock) void bucket_sum_kernel(const unsigned long long* __restrict__ vals, const unsigned* __restrict__ ids, int64_t n,
                                                             unsigned long long* __restrict__ counts, Agg agg) {
  __shared__ unsigned long long s_w[Agg::kWords * kLdsGroups];
  __shared__ unsigned s_cnt[kLdsGroups];
  agg.begin();
  const int64_t lo = (int64_t)blockIdx.x * kChunkRows, hi = lo + kChunkRows < n ? lo + kChunkRows : n;
  int64_t pos = lo;
  while (pos < hi) {
    const unsigned bucket = (ids[pos] & 0x7fffffffu) >> kBucketShift;
    // end of this window's run inside the chunk (rows are ordered by window): 256-ary search, every
    // thread probes one sample per round, the samples still inside the window form a prefix
    int64_t a = pos, span = hi - pos;
    while (span > 1) {
      const int64_t step = (span + kBlock - 1) / kBlock;
      const int64_t idx = a + (int64_t)threadIdx.x * step;
      const bool inside = idx < a + span && ((ids[idx] & 0x7fffffffu) >> kBucketShift) == bucket;
      const int cnt = __syncthreads_count(inside);  // ≥ 1: the sample of thread 0 is row a
      const int64_t lim = a + span;
      a += (int64_t)(cnt - 1) * step;
      span = lim - a < step ? lim - a : step;
    }
    const int64_t end = a + 1;
    if (end - pos < kShortRun) {
      for (int64_t i = pos + threadIdx.x; i < end; i += kBlock) {
        const unsigned id = ids[i];
        if (id & 0x80000000u) continue;  // null value: neither summed nor counted
        global_row(agg, counts, (size_t)id, vals[i]);
      }
    } else {
      lds_fill<Agg>(s_w, s_cnt, kLdsGroups);
      constexpr int U = 4;
      for (int64_t b0 = pos + threadIdx.x; b0 < end; b0 += (int64_t)kBlock * U) {
        unsigned id[U];
        unsigned long long v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
          const int64_t i = b0 + (int64_t)u * kBlock;
          id[u] = i < end ? __builtin_nontemporal_load(&ids[i]) : 0x80000000u;
          v[u] = i < end ? __builtin_nontemporal_load(&vals[i]) : 0ull;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
          if (id[u] & 0x80000000u) continue;  // null value (or past the run)
          lds_row(agg, s_w, s_cnt, (int)(id[u] & (kLdsGroups - 1)), (size_t)id[u], v[u]);
        }
      }
      lds_flush(agg, s_w, s_cnt, kLdsGroups, counts, (size_t)bucket << kBucketShift);
      __syncthreads();
    }
    pos = end;
  }
}

__global__ __launch_bounds__(kBlock) void min_max_init_kernel(unsigned long long* __restrict__ mins, unsigned long long* __restrict__ maxs,
                                                               unsigned long long* __restrict__ counts, int64_t ngroups) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g < ngroups) { mins[g] = kMinIdentity; maxs[g] = kMaxIdentity; counts[g] = 0; }
}

// ordered words → values, in place: zeros for a group without valid values, the canonical quiet NaN for a Float64 group of NaNs
template <int KIND>
__global__ __launch_bounds__(kBlock) void min_max_finish_kernel(unsigned long long* __restrict__ mins, unsigned long long* __restrict__ maxs,
                                                                 const unsigned long long* __restrict__ counts, int64_t ngroups) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= ngroups) return;
  const unsigned long long lo = mins[g], hi = maxs[g];
  unsigned long long omin, omax;
  if (counts[g] == 0) omin = omax = 0;
  else if (KIND == kF64 && lo == kMinIdentity) omin = omax = kQuietNaN;
  else { omin = from_ordered<KIND>(lo); omax = from_ordered<KIND>(hi); }
  mins[g] = omin;
  maxs[g] = omax;
}

// ---- the host side -----------------------------------------------------------------------------------------------------------------
// What a call of either aggregate starts and ends with.  check(): the argument checks and the host results of a call without rows
// (then *ids stays null).  groups(): ONE reservation of the context's temp arena — a dense group id per row in front, `extra` bytes
// of the aggregate's own behind (encode stays out of that arena) —, whatever `before` enqueues ahead of the encode, and the ids.
struct GroupCall {
  ah_ctx* c;
  const char* who;
  const uint64_t* keys;
  const uint8_t* kvalid;
  int64_t koff, n;
  uint64_t* out_keys;
  int64_t* out_first_rows;
  int64_t* out_ngroups_host;
  int32_t* out_null_group_host;
  int32_t* ids = nullptr;
  uint8_t* extra = nullptr;
  int64_t ngroups = 0;
  int32_t null_group = -1;

  int check(int64_t voff, bool buffers, bool* empty) {
    *empty = true;
    if (n < 0 || koff < 0 || voff < 0) return ah_fail(c, AH_EINVALID, "%s: negative length/offset", who);
    report();
    if (n == 0) return AH_OK;
    if (!buffers) return ah_fail(c, AH_EINVALID, "%s: null buffer", who);
    *empty = false;
    return AH_OK;
  }
  template <class Before>
  int groups(size_t extra_bytes, Before&& before) {
    void* arena = nullptr;
    int rc = ah_temp_reserve(c, ah_pad((size_t)n * 4) + extra_bytes, &arena);
    if (rc != AH_OK) return rc;
    ids = (int32_t*)arena;
    extra = (uint8_t*)arena + ah_pad((size_t)n * 4);
    if ((rc = before()) != AH_OK) return rc;
    return ah_encode_u64_groups(c, keys, kvalid, koff, n, ids, out_keys, out_first_rows, &ngroups, &null_group);
  }
  int report() {
    if (out_ngroups_host) *out_ngroups_host = ngroups;
    if (out_null_group_host) *out_null_group_host = null_group;
    return AH_OK;
  }
};

// ---- the aggregates as functions of (ids, ngroups): what ah_hash_* run behind their encode and ah_group_* run on the caller's ids -------
// The temporaries of a sum, `bytes()` of the temp arena from `base` on: above 4096 groups the partitioned (value, id) pairs with their
// histograms, sized for the two-pass partition; doubles: 128-bit fixed-point accumulators + flag word per group (room for max_groups)
// and the absmax words.
template <bool F64>
struct SumTemps {
  size_t pv, pi, ph, part_bytes, fxw, fxf;
  SumTemps(int64_t n, int64_t max_groups) {
    const int64_t nb = ah_ceil_div(n, 2048);
    pv = (size_t)n * 8; pi = ah_pad((size_t)n * 4); ph = (size_t)256 * nb * 4;
    part_bytes = 2 * (pv + pi) + 2 * ph + 256;
    // (a wide Float64 column keeps one scale word per group there: more than the pairs only when the caller's groups outnumber its rows)
    if (F64 && part_bytes < ah_pad((size_t)max_groups * 8)) part_bytes = ah_pad((size_t)max_groups * 8);
    fxw = F64 ? ah_pad((size_t)max_groups * 8) : 0; fxf = F64 ? ah_pad((size_t)max_groups * 4) : 0;
  }
  size_t bytes() const { return part_bytes + 2 * fxw + fxf + 256; }
  // doubles: the accumulators' places, and the largest finite |x| of the call enqueued (it does not need the ids)
  int begin(ah_ctx* c, uint8_t* base, const void* vals, const uint8_t* vvalid, int64_t voff, int64_t n, FxAcc* fx) const {
    *fx = FxAcc{nullptr, nullptr, nullptr, nullptr, nullptr};
    if (!F64) return AH_OK;
    uint8_t* fxbase = base + part_bytes;
    *fx = FxAcc{(unsigned long long*)fxbase, (unsigned long long*)(fxbase + fxw), (unsigned*)(fxbase + 2 * fxw),
                (const unsigned long long*)(fxbase + 2 * fxw + fxf), nullptr};
    AH_HIP(c, hipMemsetAsync((void*)fx->absmax, 0, 16, c->stream));
    absmax_kernel<<<ah_stream_grid(c, ah_ceil_div(n, (int64_t)kBlock * 8), 2), kBlock, 0, c->stream>>>((const unsigned long long*)vals, vvalid, voff, n,
                                                                                                        (unsigned long long*)fx->absmax);
    AH_LAUNCH_CHECK(c);
    return AH_OK;
  }
};

template <bool F64>   // values: Int64 / Uint64 bit patterns (wrapping sum) or doubles; `part`: the temporaries, t.begin() has run
int sum_over_ids(ah_ctx* c, const int32_t* ids, int64_t ng, const void* vals, const uint8_t* vvalid, int64_t voff, int64_t n, void* out_sums,
                 int64_t* out_counts, const SumTemps<F64>& t, uint8_t* part, FxAcc fx) {
  int rc;
  const size_t pv = t.pv, pi = t.pi, ph = t.ph;
  AH_HIP(c, hipMemsetAsync(out_sums, 0, (size_t)ng * 8, c->stream));
  AH_HIP(c, hipMemsetAsync(out_counts, 0, (size_t)ng * sizeof(int64_t), c->stream));
  bool wide = false;
  if (F64) {
    AH_HIP(c, hipMemsetAsync(fx.lo, 0, (size_t)ng * 8, c->stream));
    AH_HIP(c, hipMemsetAsync(fx.hi, 0, (size_t)ng * 8, c->stream));
    AH_HIP(c, hipMemsetAsync(fx.flags, 0, (size_t)ng * 4, c->stream));
    // one scale for the call, or one per group?  (ah_hashing.h: a column spanning more than 42 binades)
    AH_HIP(c, hipMemcpyAsync(&c->pinned[2], fx.absmax, 16, hipMemcpyDeviceToHost, c->stream));
    AH_HIP(c, hipStreamSynchronize(c->stream));
    wide = fx_wide(*(volatile uint64_t*)&c->pinned[2], *(volatile uint64_t*)&c->pinned[3]);
    if (wide) {
      unsigned long long* gmax = (unsigned long long*)part;   // the partition temporaries are idle on this route
      AH_HIP(c, hipMemsetAsync(gmax, 0, (size_t)ng * 8, c->stream));
      if ((rc = group_agg(c, ids, vals, vvalid, voff, n, nullptr, ng, AbsMax{gmax})) != AH_OK) return rc;
      fx.gmax = gmax;
    }
  }
  auto aggregate = [&](auto agg) -> int {
    if (ng <= kLdsGroups || !c->opt_hash_sum_partition || wide || ng > kPartitionMaxGroups)
      return group_agg(c, ids, vals, vvalid, voff, n, out_counts, ng, agg);
    const int passes = ng <= kPartitionOnePass ? 1 : 2;
    unsigned long long* pvals = (unsigned long long*)part;
    unsigned* pids = (unsigned*)(part + pv);
    unsigned* hist = (unsigned*)(part + pv + pi);
    unsigned* offs = (unsigned*)(part + pv + pi + ph);
    unsigned long long* avals = passes == 2 ? (unsigned long long*)(part + pv + pi + 2 * ph) : nullptr;
    unsigned* aids = passes == 2 ? (unsigned*)((uint8_t*)avals + pv) : nullptr;
    int prc = ah_partition_by_group(c, ids, (const unsigned long long*)vals, vvalid, voff, n, kBucketShift, passes, hist, offs, avals, aids, pvals, pids);
    if (prc != AH_OK) return prc;
    bucket_sum_kernel<<<(unsigned)ah_ceil_div(n, kChunkRows), kBlock, 0, c->stream>>>(pvals, pids, n, (unsigned long long*)out_counts, agg);
    AH_LAUNCH_CHECK(c);
    return AH_OK;
  };
  if constexpr (F64) {
    if ((rc = aggregate(SumF64{fx, 0})) != AH_OK) return rc;
    if (ng > 0) {
      fx_finalize_kernel<<<(unsigned)ah_ceil_div(ng, kBlock), kBlock, 0, c->stream>>>(fx, ng, (double*)out_sums);
      AH_LAUNCH_CHECK(c);
    }
  } else {
    if ((rc = aggregate(SumI64{(unsigned long long*)out_sums})) != AH_OK) return rc;
  }
  return AH_OK;
}

template <int KIND>
int min_max_over_ids(ah_ctx* c, const int32_t* ids, int64_t ng, const void* vals, const uint8_t* vvalid, int64_t voff, int64_t n, void* out_mins,
                     void* out_maxs, int64_t* out_counts) {
  if (ng <= 0) return AH_OK;
  unsigned long long *mins = (unsigned long long*)out_mins, *maxs = (unsigned long long*)out_maxs, *counts = (unsigned long long*)out_counts;
  const unsigned gblocks = (unsigned)ah_ceil_div(ng, kBlock);
  min_max_init_kernel<<<gblocks, kBlock, 0, c->stream>>>(mins, maxs, counts, ng);
  AH_LAUNCH_CHECK(c);
  if (int rc = group_agg(c, ids, vals, vvalid, voff, n, counts, ng, MinMax<KIND>{mins, maxs})) return rc;
  min_max_finish_kernel<KIND><<<gblocks, kBlock, 0, c->stream>>>(mins, maxs, counts, ng);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

template <bool F64>
int hash_sum(ah_ctx* c, const uint64_t* keys, const uint8_t* kvalid, int64_t koff, const void* vals, const uint8_t* vvalid,
             int64_t voff, int64_t n, uint64_t* out_keys, void* out_sums, int64_t* out_counts, int64_t* out_first_rows,
             int64_t* out_ngroups_host, int32_t* out_null_group_host) {
  GroupCall call{c, "hash_sum", keys, kvalid, koff, n, out_keys, out_first_rows, out_ngroups_host, out_null_group_host};
  bool empty;
  int rc = call.check(voff, keys && vals && out_keys && out_sums && out_counts, &empty);
  if (rc != AH_OK || empty) return rc;
  {
    // large inputs with up to ~10^6 groups: cut the rows by key hash first, aggregate each partition in LDS (ah_groupby.hip)
    int used = 0;
    rc = ah_groupby_partitioned_try(c, F64 ? 1 : 0, keys, kvalid, koff, vals, vvalid, voff, n, out_keys, out_sums, out_counts, out_first_rows,
                                    &call.ngroups, &call.null_group, &used);
    if (rc != AH_OK) return rc;
    if (used) return call.report();
  }
  const SumTemps<F64> t(n, n + 1);   // ≤ n + 1 groups
  FxAcc fx;
  rc = call.groups(t.bytes(), [&]() -> int { return t.begin(c, call.extra, vals, vvalid, voff, n, &fx); });
  if (rc != AH_OK) return rc;
  if ((rc = sum_over_ids<F64>(c, call.ids, call.ngroups, vals, vvalid, voff, n, out_sums, out_counts, t, call.extra, fx)) != AH_OK) return rc;
  return call.report();
}

// group-by min / max: the same groups as hash_sum
template <int KIND>
int hash_min_max(ah_ctx* c, const uint64_t* keys, const uint8_t* kvalid, int64_t koff, const void* vals, const uint8_t* vvalid,
                 int64_t voff, int64_t n, uint64_t* out_keys, void* out_mins, void* out_maxs, int64_t* out_counts, int64_t* out_first_rows,
                 int64_t* out_ngroups_host, int32_t* out_null_group_host) {
  GroupCall call{c, "hash_min_max", keys, kvalid, koff, n, out_keys, out_first_rows, out_ngroups_host, out_null_group_host};
  bool empty;
  int rc = call.check(voff, keys && vals && out_keys && out_mins && out_maxs && out_counts, &empty);
  if (rc != AH_OK || empty) return rc;
  if ((rc = call.groups(0, [] { return AH_OK; })) != AH_OK) return rc;
  if ((rc = min_max_over_ids<KIND>(c, call.ids, call.ngroups, vals, vvalid, voff, n, out_mins, out_maxs, out_counts)) != AH_OK) return rc;
  return call.report();
}

// ---- the same aggregates over the caller's ids (ah_group_*): 0 ≤ ids[i] < ngroups is the caller's word (group_agg_kernel leaves a row
// that breaks it out, the partitioned sum above 4096 groups trusts it)
int group_check(ah_ctx* c, const char* who, int64_t ngroups, int64_t voff, int64_t n, bool buffers, bool* nothing) {
  *nothing = true;
  if (n < 0 || voff < 0 || ngroups < 0) return ah_fail(c, AH_EINVALID, "%s: negative length/offset", who);
  if (ngroups > 0x7fffffffll) return ah_fail(c, AH_EINVALID, "%s: more than 2^31 - 1 groups", who);
  if (n > ((int64_t)1 << 30)) return ah_fail(c, AH_ENOTIMPL, "%s: more than 2^30 rows per call", who);
  if (ngroups == 0) return AH_OK;
  if (!buffers) return ah_fail(c, AH_EINVALID, "%s: null buffer", who);
  *nothing = false;
  return AH_OK;
}

template <bool F64>
int group_sum(ah_ctx* c, const int32_t* ids, int64_t ngroups, const void* vals, const uint8_t* vvalid, int64_t voff, int64_t n, void* out_sums,
              int64_t* out_counts) {
  bool nothing;
  int rc = group_check(c, "group_sum", ngroups, voff, n, out_sums && out_counts && (n == 0 || (ids && vals)), &nothing);
  if (rc != AH_OK || nothing) return rc;
  if (n == 0) {   // no rows: every group is empty
    AH_HIP(c, hipMemsetAsync(out_sums, 0, (size_t)ngroups * 8, c->stream));
    AH_HIP(c, hipMemsetAsync(out_counts, 0, (size_t)ngroups * sizeof(int64_t), c->stream));
    return AH_OK;
  }
  const SumTemps<F64> t(n, ngroups);
  void* arena = nullptr;
  if ((rc = ah_temp_reserve(c, t.bytes(), &arena)) != AH_OK) return rc;
  FxAcc fx;
  if ((rc = t.begin(c, (uint8_t*)arena, vals, vvalid, voff, n, &fx)) != AH_OK) return rc;
  return sum_over_ids<F64>(c, ids, ngroups, vals, vvalid, voff, n, out_sums, out_counts, t, (uint8_t*)arena, fx);
}

template <int KIND>
int group_min_max(ah_ctx* c, const int32_t* ids, int64_t ngroups, const void* vals, const uint8_t* vvalid, int64_t voff, int64_t n, void* out_mins,
                  void* out_maxs, int64_t* out_counts) {
  bool nothing;
  int rc = group_check(c, "group_min_max", ngroups, voff, n, out_mins && out_maxs && out_counts && (n == 0 || (ids && vals)), &nothing);
  if (rc != AH_OK || nothing) return rc;
  return min_max_over_ids<KIND>(c, ids, ngroups, vals, vvalid, voff, n, out_mins, out_maxs, out_counts);
}

}  // namespace

AH_EXPORT int ah_hash_sum_f64(ah_ctx* c, const uint64_t* keys, const uint8_t* kvalid, int64_t koff,
                              const double* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                              uint64_t* out_keys, double* out_sums, int64_t* out_counts, int64_t* out_first_rows,
                              int64_t* out_ngroups_host, int32_t* out_null_group_host) {
  AH_ENTER(c);
  return hash_sum<true>(c, keys, kvalid, koff, vals, vvalid, voff, n, out_keys, out_sums, out_counts, out_first_rows, out_ngroups_host, out_null_group_host);
}

AH_EXPORT int ah_hash_sum_i64(ah_ctx* c, const uint64_t* keys, const uint8_t* kvalid, int64_t koff,
                              const int64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                              uint64_t* out_keys, int64_t* out_sums, int64_t* out_counts, int64_t* out_first_rows,
                              int64_t* out_ngroups_host, int32_t* out_null_group_host) {
  AH_ENTER(c);
  return hash_sum<false>(c, keys, kvalid, koff, vals, vvalid, voff, n, out_keys, out_sums, out_counts, out_first_rows, out_ngroups_host, out_null_group_host);
}

AH_EXPORT int ah_hash_min_max_i64(ah_ctx* c, const uint64_t* keys, const uint8_t* kvalid, int64_t koff,
                                  const int64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                                  uint64_t* out_keys, int64_t* out_mins, int64_t* out_maxs, int64_t* out_counts, int64_t* out_first_rows,
                                  int64_t* out_ngroups_host, int32_t* out_null_group_host) {
  AH_ENTER(c);
  return hash_min_max<kI64>(c, keys, kvalid, koff, vals, vvalid, voff, n, out_keys, out_mins, out_maxs, out_counts, out_first_rows,
                            out_ngroups_host, out_null_group_host);
}

AH_EXPORT int ah_hash_min_max_u64(ah_ctx* c, const uint64_t* keys, const uint8_t* kvalid, int64_t koff,
                                  const uint64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                                  uint64_t* out_keys, uint64_t* out_mins, uint64_t* out_maxs, int64_t* out_counts, int64_t* out_first_rows,
                                  int64_t* out_ngroups_host, int32_t* out_null_group_host) {
  AH_ENTER(c);
  return hash_min_max<kU64>(c, keys, kvalid, koff, vals, vvalid, voff, n, out_keys, out_mins, out_maxs, out_counts, out_first_rows,
                            out_ngroups_host, out_null_group_host);
}

AH_EXPORT int ah_hash_min_max_f64(ah_ctx* c, const uint64_t* keys, const uint8_t* kvalid, int64_t koff,
                                  const double* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                                  uint64_t* out_keys, double* out_mins, double* out_maxs, int64_t* out_counts, int64_t* out_first_rows,
                                  int64_t* out_ngroups_host, int32_t* out_null_group_host) {
  AH_ENTER(c);
  return hash_min_max<kF64>(c, keys, kvalid, koff, vals, vvalid, voff, n, out_keys, out_mins, out_maxs, out_counts, out_first_rows,
                            out_ngroups_host, out_null_group_host);
}

AH_EXPORT int ah_group_sum_i64(ah_ctx* c, const int32_t* ids, int64_t ngroups, const int64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                               int64_t* out_sums, int64_t* out_counts) {
  AH_ENTER(c);
  return group_sum<false>(c, ids, ngroups, vals, vvalid, voff, n, out_sums, out_counts);
}

AH_EXPORT int ah_group_sum_f64(ah_ctx* c, const int32_t* ids, int64_t ngroups, const double* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                               double* out_sums, int64_t* out_counts) {
  AH_ENTER(c);
  return group_sum<true>(c, ids, ngroups, vals, vvalid, voff, n, out_sums, out_counts);
}

AH_EXPORT int ah_group_min_max_i64(ah_ctx* c, const int32_t* ids, int64_t ngroups, const int64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                                   int64_t* out_mins, int64_t* out_maxs, int64_t* out_counts) {
  AH_ENTER(c);
  return group_min_max<kI64>(c, ids, ngroups, vals, vvalid, voff, n, out_mins, out_maxs, out_counts);
}

AH_EXPORT int ah_group_min_max_u64(ah_ctx* c, const int32_t* ids, int64_t ngroups, const uint64_t* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                                   uint64_t* out_mins, uint64_t* out_maxs, int64_t* out_counts) {
  AH_ENTER(c);
  return group_min_max<kU64>(c, ids, ngroups, vals, vvalid, voff, n, out_mins, out_maxs, out_counts);
}

AH_EXPORT int ah_group_min_max_f64(ah_ctx* c, const int32_t* ids, int64_t ngroups, const double* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                                   double* out_mins, double* out_maxs, int64_t* out_counts) {
  AH_ENTER(c);
  return group_min_max<kF64>(c, ids, ngroups, vals, vvalid, voff, n, out_mins, out_maxs, out_counts);
}
