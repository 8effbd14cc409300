// ah_varout.h — the tail every producer of a var-length output shares (host side; internal): the Take of ah_varlen.hip, the if_else
// of ah_conditional.hip, the formatted casts of ah_cast_string.hip, the ranges of ah_string_transform.hip.  Each brings its own
// lengths kernel, argument checks and error texts; the rest is here, in three pieces around that kernel:
//   varout_begin    lens and incl (n 8-byte words each) in the temp arena — the scan takes the scratch arena —, the caller's own
//                   region in the same reservation, the overflow flag (and the count word in front of it) zeroed;
//   varout_enqueue  lengths → inclusive scan (ah_cumulative_sum) → offsets_kernel → the results to pinned memory;
//   varout_finish   the call's one synchronisation; the byte total and the overflow flag.
// One pinned layout for everyone, kVarPin*: words 0 … 2 mirror dscalars[1 … 3] — what a lengths kernel may leave in [1] and [2] is
// its caller's (Take: the first bad position, the count of valid rows) and comes home in the same synchronisation —, word 3 is the
// total.
// n = 0 is the callers' business and they differ: Take, if_else and the formatted cast write the lone closing offset, ah_string_ranges
// touches nothing (include/arrowhip_strings.h says so).
#pragma once
#include "ah_common.h"

namespace {

// out_offsets[0] = 0, out_offsets[i + 1] = incl[i]; int32 offsets: flag an overflow
template <typename OffT, int BLOCK>
__global__ __launch_bounds__(BLOCK) void offsets_kernel(const long long* __restrict__ incl, int64_t n, OffT* __restrict__ out_offsets,
                                                         unsigned* __restrict__ overflow) {
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i <= n; i += stride) {
    const long long v = i == 0 ? 0 : incl[i - 1];
    if (sizeof(OffT) == 4 && v > 2147483647ll) atomicOr(overflow, 1u);
    out_offsets[i] = (OffT)v;
  }
}

constexpr int kDsVarFirst = 1, kDsVarCount = 2, kDsVarOverflow = 3;                  // words of dscalars
constexpr int kVarPinFirst = 0, kVarPinCount = 1, kVarPinOverflow = 2, kVarPinTotal = 3;   // words of pinned

struct VarOut {
  long long* lens;   // [0, n): the caller's lengths kernel writes them
  long long* incl;   // their inclusive scan
  void* extra;       // the caller's own bytes
  bool can_overflow;
};

// can_overflow = false: the caller's lengths cannot exceed the offset type (a result never longer than its input row) — the overflow
// word is neither zeroed nor brought home, and varout_finish reports none.  Else words [2] and [3] of dscalars are zeroed.
inline int varout_begin(ah_ctx* c, int64_t n, size_t extra_bytes, bool can_overflow, VarOut* v) {
  const size_t col = ah_pad((size_t)n * 8), ext = ah_pad(extra_bytes);
  void* arena = nullptr;
  if (int rc = ah_temp_reserve(c, ext + 2 * col, &arena)) return rc;
  v->extra = arena;
  v->lens = (long long*)((uint8_t*)arena + ext);
  v->incl = (long long*)((uint8_t*)arena + ext + col);
  v->can_overflow = can_overflow;
  if (can_overflow) AH_HIP(c, hipMemsetAsync(&c->dscalars[kDsVarCount], 0, 2 * sizeof(uint64_t), c->stream));
  return AH_OK;
}

// caller_words: dscalars[1] and [2] come home with the overflow flag, in the one copy
inline int varout_enqueue(ah_ctx* c, const VarOut& v, int64_t n, int offset_width, void* out_offsets, bool caller_words) {
  constexpr int kBlock = 256;
  if (int rc = ah_cumulative_sum(c, AH_INT64, v.lens, nullptr, 0, n, nullptr, 0, 0, v.incl, nullptr, nullptr)) return rc;
  const unsigned grid = ah_stream_grid(c, ah_ceil_div(n + 1, kBlock), 8);
  unsigned* overflow = (unsigned*)&c->dscalars[kDsVarOverflow];
  if (offset_width == 4) offsets_kernel<int32_t, kBlock><<<grid, kBlock, 0, c->stream>>>(v.incl, n, (int32_t*)out_offsets, overflow);
  else offsets_kernel<long long, kBlock><<<grid, kBlock, 0, c->stream>>>(v.incl, n, (long long*)out_offsets, overflow);
  AH_LAUNCH_CHECK(c);
  const int first = caller_words ? kDsVarFirst : kDsVarOverflow;
  if (v.can_overflow)
    AH_HIP(c, hipMemcpyAsync(&c->pinned[kVarPinFirst + first - kDsVarFirst], &c->dscalars[first], (size_t)(kDsVarOverflow + 1 - first) * sizeof(uint64_t),
                             hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipMemcpyAsync(&c->pinned[kVarPinTotal], v.incl + n - 1, 8, hipMemcpyDeviceToHost, c->stream));
  return AH_OK;
}

inline int varout_finish(ah_ctx* c, const VarOut& v, int64_t* total, bool* overflow) {
  AH_HIP(c, hipStreamSynchronize(c->stream));
  *total = *(volatile int64_t*)&c->pinned[kVarPinTotal];
  *overflow = v.can_overflow && (*(volatile unsigned*)&c->pinned[kVarPinOverflow] & 1u);
  return AH_OK;
}

}  // namespace
