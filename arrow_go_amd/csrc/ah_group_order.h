// ah_group_order.h — the order-preserving 64-bit words of the group-by min / max (ah_hash_agg.hip, ah_group_agg.hip) and the look
// before the atomic that both translation units put in front of atomicMin / atomicMax.
#pragma once
#include "ah_common.h"

namespace {

// Every value is mapped to an unsigned 64-bit word whose unsigned order is the value's order — u64: itself; i64: sign bit flipped; f64:
// negative → all bits flipped, else sign bit set (so −0 → 0x7FFF…F < +0 → 0x8000…0, −inf lowest, +inf highest).  Minimum and maximum
// are then atomicMin / atomicMax on unsigned long long, in LDS and in HBM, and commute: the result is a function of the inputs alone,
// whatever the order of arrival and whichever regime ran.  A NaN row is counted and issues no update.  The accumulators start at the
// identities (min: all ones, max: zero); all ones is the image of no non-NaN double, so a Float64 group with count > 0 whose minimum is
// still the identity held NaNs only.  The accumulators ARE out_mins / out_maxs: the finishing kernel un-maps them in place.
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
// at workgroup scope (a plain ds_read).  The slot only ever moves towards the row's side, so a stale look costs an atomic, never an
// update; ids are dense and values arrive in no order, so after the first few rows of a group almost no row issues one.
__device__ __forceinline__ unsigned long long look(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long look_lds(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

}  // namespace
