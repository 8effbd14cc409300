// ah_reduce.h — the streaming-reduction layer ("Streaming reductions"): what Sum (ah_sum.hip), the fused Compare → Filter → Sum
// (ah_fused.hip), min_max (ah_minmax.hip), the popcount (ah_bitmap.hip) and the sort's key statistics (ah_sort_radix.h,
// ah_sort.hip) share.  Plain templates, every functor inlined, no run-time option.
//
//   split    a column = ≤ 1 vector of head rows, a 16-byte-aligned body of nvec vectors, ≤ 1 vector of tail rows
//   walk     grid-stride over the body, kReduceUnroll 16-byte loads in flight per lane (hinted or plain: a template flag)
//   classed  the Float64 rule of ah_ddsum.h: walk fast, remember the largest high word, walk again classed if a wave met a big row
//   part     a trivially copyable struct with init() — the start value — and merge(const Part&); lanes → wave → workgroup → finish
//   finish   the second launch: one workgroup merges the per-workgroup partials and hands the result to an Emit functor
#pragma once
#include "ah_common.h"
#include "ah_ddsum.h"

constexpr int kReduceBlock = 256;
constexpr int kReduceUnroll = 4;   // 16-byte loads in flight per lane

// ---- alignment split ---------------------------------------------------------------------------------------------------------
struct ah_split {
  int64_t head, nvec, tail;   // rows, 16-byte vectors, rows
};
template <typename T>
__host__ __device__ inline ah_split ah_reduce_split(const T* p, int64_t n) {
  constexpr int64_t V = 16 / sizeof(T);
  int64_t head = (int64_t)(((16 - ((uintptr_t)p & 15)) & 15) / sizeof(T));
  if (head > n) head = n;
  const int64_t nvec = (n - head) / V;
  return ah_split{head, nvec, n - head - nvec * V};
}

#if defined(__HIPCC__)
// ---- the walk ----------------------------------------------------------------------------------------------------------------
// Full iterations: all kReduceUnroll loads issued before any use, f(j, v) for vector j.  One ragged last iteration: guarded plain
// loads, g(j, v).  The functors own their accumulators; a lane sees its vectors in ascending j (part of a Float64 sum's low bits).
template <typename Vec, bool NT, typename F, typename G>
__device__ __forceinline__ void ah_reduce_walk(const Vec* __restrict__ body, int64_t nvec, F&& f, G&& g) {
  const int64_t stride = (int64_t)gridDim.x * kReduceBlock * kReduceUnroll;
  int64_t i = (int64_t)blockIdx.x * kReduceBlock * kReduceUnroll + threadIdx.x;
  for (; i + (int64_t)(kReduceUnroll - 1) * kReduceBlock < nvec; i += stride) {
    Vec v[kReduceUnroll];
#pragma unroll
    for (int k = 0; k < kReduceUnroll; k++) {
      if (NT) v[k] = __builtin_nontemporal_load(&body[i + (int64_t)k * kReduceBlock]);
      else v[k] = body[i + (int64_t)k * kReduceBlock];
    }
#pragma unroll
    for (int k = 0; k < kReduceUnroll; k++) f(i + (int64_t)k * kReduceBlock, v[k]);
  }
#pragma unroll
  for (int k = 0; k < kReduceUnroll; k++) {
    const int64_t j = i + (int64_t)k * kReduceBlock;
    if (j < nvec) g(j, body[j]);
  }
}
template <typename Vec, bool NT, typename F>
__device__ __forceinline__ void ah_reduce_walk(const Vec* __restrict__ body, int64_t nvec, F&& f) {
  ah_reduce_walk<Vec, NT>(body, nvec, f, f);
}

// The classed Float64 rule.  fast(j, v) takes every row for an ordinary one (the unguarded TwoSum: nothing branches inside the
// loop) and returns the largest high word, sign cleared, among the rows it added; careful(j, v) classes every row (ah_ddx_add).
// A wave in which some lane met a row ≥ 2^960, ±inf or NaN throws its sums away — reset() — and walks its share again with
// careful: an ordinary column never takes a branch, a column with a few special rows re-reads the shares of the few waves that
// met them, a column full of them costs two reads.  The ragged iteration is careful from the start.  CLASSED = false (integers
// have one class): one careful walk.
template <typename Vec, bool NT, bool CLASSED, typename Fast, typename Careful, typename Reset>
__device__ __forceinline__ void ah_reduce_walk_classed(const Vec* __restrict__ body, int64_t nvec, Fast&& fast, Careful&& careful, Reset&& reset) {
  if constexpr (CLASSED) {
    unsigned top = 0;
    ah_reduce_walk<Vec, NT>(body, nvec, [&](int64_t j, const Vec& v) { top = max(top, fast(j, v)); }, careful);
    if (__any(top >= AH_DDX_BIG_HI)) {   // wave-uniform
      reset();
      ah_reduce_walk<Vec, NT>(body, nvec, careful);
    }
  } else {
    ah_reduce_walk<Vec, NT>(body, nvec, careful);
  }
}

// ---- parts -------------------------------------------------------------------------------------------------------------------
struct ah_sum_u64 {   // wrapping integer sum, popcount
  unsigned long long s;
  __device__ __forceinline__ void init() { s = 0; }
  __device__ __forceinline__ void merge(const ah_sum_u64& o) { s += o.s; }
};

// lane l takes lane l + o's part, 32 bits at a time
template <typename Part>
__device__ __forceinline__ Part ah_shfl_down_part(const Part& p, int o) {
  static_assert(std::is_trivially_copyable<Part>::value, "a part travels as words");
  constexpr int W = (int)((sizeof(Part) + 3) / 4);
  unsigned w[W] = {};
  __builtin_memcpy(w, &p, sizeof(Part));
#pragma unroll
  for (int k = 0; k < W; k++) w[k] = __shfl_down(w[k], o, 64);
  Part r;
  __builtin_memcpy(&r, w, sizeof(Part));
  return r;
}
// the wave's parts merged down the o = 32 … 1 tree; valid in lane 0
template <typename Part>
__device__ __forceinline__ Part ah_wave_reduce(Part p) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) p.merge(ah_shfl_down_part(p, o));
  return p;
}
// the workgroup's parts: wave reduce, one LDS slot per wave, thread 0 merges sm[0], sm[1], … in that order; valid in thread 0.
// ONCE per kernel and part type: the slots belong to the instantiation, and a second call with the same Part would write
// them with no barrier behind the first call's reads (no kernel here reduces twice; one that does puts a __syncthreads between).
template <int BLOCK, typename Part>
__device__ __forceinline__ Part ah_block_reduce(Part p) {
  __shared__ Part sm[BLOCK / 64];
  p = ah_wave_reduce(p);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    p = sm[0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; w++) p.merge(sm[w]);
  }
  return p;
}

// ---- the finish --------------------------------------------------------------------------------------------------------------
// One workgroup: partials[0 .. n) strided over the block, reduced, emit(result) in thread 0.  The caller owns the partials.
template <typename Part, typename Emit>
__global__ __launch_bounds__(kReduceBlock) void ah_reduce_finish_kernel(const Part* __restrict__ partials, int n, Emit emit) {
  Part a;
  a.init();
  for (int i = threadIdx.x; i < n; i += kReduceBlock) a.merge(partials[i]);
  a = ah_block_reduce<kReduceBlock>(a);
  if (threadIdx.x == 0) emit(a);
}
template <typename Part, typename Emit>
inline int ah_reduce_finish(ah_ctx* c, const Part* partials, int n, Emit emit) {
  ah_reduce_finish_kernel<Part, Emit><<<1, kReduceBlock, 0, c->stream>>>(partials, n, emit);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}
// The two launches over the scratch arena: `iters` walk iterations → grid (ah_stream_grid), one partial per workgroup in
// scratch, first(grid, partials) launches the kernel that reads the column, the finish follows.
template <typename Part, typename First, typename Emit>
inline int ah_reduce_two_launch(ah_ctx* c, int64_t iters, int default_bpc, First&& first, Emit emit) {
  const unsigned grid = ah_stream_grid(c, iters, default_bpc);
  void* scratch;
  int rc = ah_scratch_reserve(c, (size_t)grid * sizeof(Part), &scratch);
  if (rc != AH_OK) return rc;
  first(grid, (Part*)scratch);
  AH_LAUNCH_CHECK(c);
  return ah_reduce_finish(c, (const Part*)scratch, (int)grid, emit);
}
#endif
