// ah_hash_minmax.hip — per-group minimum, maximum and count over dense group ids (the aggregate behind ah_hash_min_max_*).
//
// No reference analogue (arrow-go has no hash aggregate); definition in DESIGN.md §3.2.  ah_hash.hip produces the ids
// (dictionary_encode, first-seen order) and calls ah_group_min_max below.
//
// Every value is mapped to an unsigned 64-bit word whose unsigned order is the value's order — u64: itself; i64: sign bit
// flipped; f64: negative → all bits flipped, else sign bit set (so −0 → 0x7FFF…F < +0 → 0x8000…0, −inf lowest, +inf highest).
// Minimum and maximum are then atomicMin / atomicMax on unsigned long long, in LDS and in HBM, and commute: the result is a
// function of the inputs alone, whatever the order of arrival and whichever regime ran.  A NaN row is counted and issues no
// update.  The accumulators start at the identities (min: all ones, max: zero); all ones is the image of no non-NaN double, so
// a Float64 group with count > 0 whose minimum is still the identity held NaNs only.  The accumulators ARE out_mins / out_maxs:
// the finishing kernel un-maps them in place.
//
// Regimes, by the number of groups (as the group-by sum, ah_hash.hip):
//   ≤ 4096   every workgroup keeps {min, max, count} of all groups in LDS (4096 × 20 B = 80 KiB, two workgroups per CU); a row
//            reads its group's slot and issues the LDS atomic only when it improves it — ids are dense and values arrive in no
//            order, so after the first few rows of a group almost none does; one flush per touched group, again behind a look.
//   > 4096   device atomics straight into the outputs behind a relaxed device-scope load (the look of ah_hash.hip's
//            group_max_kernel), and one device atomic per row for the count.
// HBM: 12 B/row (id + value) + the validity bits.
#include "ah_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kLdsGroups = 4096;   // as ah_hash.hip's group_sum_kernel
constexpr unsigned long long kMinIdentity = ~0ull, kMaxIdentity = 0ull;
constexpr unsigned long long kSignBit = 0x8000000000000000ull;
constexpr unsigned long long kQuietNaN = 0x7FF8000000000000ull;

enum : int { kU64 = 0, kI64 = 1, kF64 = 2 };

template <int KIND>
__device__ __forceinline__ unsigned long long to_ordered(unsigned long long bits) {
  if constexpr (KIND == kU64) return bits;
  else if constexpr (KIND == kI64) return bits ^ kSignBit;
  else return (bits & kSignBit) ? ~bits : bits | kSignBit;
}
template <int KIND>
__device__ __forceinline__ unsigned long long from_ordered(unsigned long long w) {
  if constexpr (KIND == kU64) return w;
  else if constexpr (KIND == kI64) return w ^ kSignBit;
  else return (w & kSignBit) ? w ^ kSignBit : ~w;
}
template <int KIND>
__device__ __forceinline__ bool is_nan_bits(unsigned long long bits) {
  return KIND == kF64 && (bits & ~kSignBit) > 0x7FF0000000000000ull;
}

// the look before the atomic: a relaxed load — of an HBM slot at device scope (served by L2, where the atomics execute), of an LDS slot
// at workgroup scope (a plain ds_read).  The slot only ever moves towards the row's side, so a stale look costs an atomic, never an update.
__device__ __forceinline__ unsigned long long look(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long look_lds(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// mins / maxs hold the identities, counts zeros, for all `ngroups` groups when this starts.
template <int KIND, bool USE_LDS>
__global__ __launch_bounds__(kBlock) void group_min_max_kernel(const int32_t* __restrict__ ids, const unsigned long long* __restrict__ vals,
                                                                const uint8_t* __restrict__ vvalid, int64_t voff, int64_t n,
                                                                unsigned long long* __restrict__ mins, unsigned long long* __restrict__ maxs,
                                                                unsigned long long* __restrict__ counts, int ngroups) {
  __shared__ unsigned long long s_min[USE_LDS ? kLdsGroups : 1];
  __shared__ unsigned long long s_max[USE_LDS ? kLdsGroups : 1];
  __shared__ unsigned s_cnt[USE_LDS ? kLdsGroups : 1];
  const int nl = ngroups < kLdsGroups ? ngroups : kLdsGroups;
  if (USE_LDS) {
    for (int g = threadIdx.x; g < nl; g += kBlock) { s_min[g] = kMinIdentity; s_max[g] = kMaxIdentity; s_cnt[g] = 0; }
    __syncthreads();
  }
  constexpr int U = 8;  // rows per lane per step: 8 id loads + 8 value loads in flight
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
      if (g[u] < 0 || g[u] >= ngroups) continue;   // (ids are < ngroups: the bound keeps a wrong id out of memory it does not own)
      const bool nan = is_nan_bits<KIND>(v[u]);
      const unsigned long long w = to_ordered<KIND>(v[u]);
      if (USE_LDS) {
        if (!nan) {
          if (w < look_lds(&s_min[g[u]])) atomicMin(&s_min[g[u]], w);
          if (w > look_lds(&s_max[g[u]])) atomicMax(&s_max[g[u]], w);
        }
        atomicAdd(&s_cnt[g[u]], 1u);
      } else {
        if (!nan) {
          if (w < look(&mins[g[u]])) atomicMin(&mins[g[u]], w);
          if (w > look(&maxs[g[u]])) atomicMax(&maxs[g[u]], w);
        }
        atomicAdd(&counts[g[u]], 1ull);
      }
    }
  }
  if (USE_LDS) {
    __syncthreads();
    for (int g = threadIdx.x; g < nl; g += kBlock) {
      const unsigned cnt = s_cnt[g];
      if (cnt) {
        const unsigned long long lo = s_min[g], hi = s_max[g];
        if (lo < look(&mins[g])) atomicMin(&mins[g], lo);
        if (hi > look(&maxs[g])) atomicMax(&maxs[g], hi);
        atomicAdd(&counts[g], (unsigned long long)cnt);
      }
    }
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

template <int KIND>
int group_min_max(ah_ctx* c, const int32_t* ids, const unsigned long long* vals, const uint8_t* vvalid, int64_t voff, int64_t n, int64_t ngroups,
                  unsigned long long* mins, unsigned long long* maxs, unsigned long long* counts) {
  const unsigned gblocks = (unsigned)ah_ceil_div(ngroups, kBlock);
  min_max_init_kernel<<<gblocks, kBlock, 0, c->stream>>>(mins, maxs, counts, ngroups);
  AH_LAUNCH_CHECK(c);
  const int ng = (int)(ngroups > 0x7fffffff ? 0x7fffffff : ngroups);
  if (ngroups <= kLdsGroups) {
    const unsigned grid = ah_stream_grid(c, ah_ceil_div(n, (int64_t)kBlock * 8), /*default_bpc=*/2);
    group_min_max_kernel<KIND, true><<<grid, kBlock, 0, c->stream>>>(ids, vals, vvalid, voff, n, mins, maxs, counts, ng);
  } else {
    const unsigned grid = ah_stream_grid(c, ah_ceil_div(n, (int64_t)kBlock * 8));
    group_min_max_kernel<KIND, false><<<grid, kBlock, 0, c->stream>>>(ids, vals, vvalid, voff, n, mins, maxs, counts, ng);
  }
  AH_LAUNCH_CHECK(c);
  min_max_finish_kernel<KIND><<<gblocks, kBlock, 0, c->stream>>>(mins, maxs, counts, ngroups);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

}  // namespace

int ah_group_min_max(ah_ctx* c, int kind, const int32_t* ids, const void* vals, const uint8_t* vvalid, int64_t voff, int64_t n, int64_t ngroups,
                     void* out_mins, void* out_maxs, int64_t* out_counts) {
  if (ngroups <= 0) return AH_OK;
  const unsigned long long* v = (const unsigned long long*)vals;
  unsigned long long *lo = (unsigned long long*)out_mins, *hi = (unsigned long long*)out_maxs, *cnt = (unsigned long long*)out_counts;
  switch (kind) {
    case kU64: return group_min_max<kU64>(c, ids, v, vvalid, voff, n, ngroups, lo, hi, cnt);
    case kI64: return group_min_max<kI64>(c, ids, v, vvalid, voff, n, ngroups, lo, hi, cnt);
    case kF64: return group_min_max<kF64>(c, ids, v, vvalid, voff, n, ngroups, lo, hi, cnt);
  }
  return ah_fail(c, AH_EINVALID, "hash_min_max: unknown value kind %d", kind);
}
