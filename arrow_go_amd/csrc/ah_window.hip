// ah_window.hip — window functions: ranks and running aggregates over the partitions of a sort order.
//
// No reference analogue (arrow-go has no window operator).  The caller brings the two expensive halves — dense partition ids
// (ah_group_ids) and the stable order of (partition id, order keys) (ah_sort_indices_keys) — and this file adds what was missing:
//   ah_window_flags   one byte per SORTED position: bit 0 "a partition starts here", bit 1 "a peer group starts here";
//   ah_window_rank    row_number / rank / dense_rank from the flags;
//   ah_window_scan    running sum / min / max / count of a value column gathered through the order.
// Everything after the flags is ONE segmented inclusive scan over the sorted positions, scattered back to the rows:
// out[order[p]] = the scan at position p.  The scan element is the pair (f, a) = ("a segment started at or before here, within
// the range this pair stands for", the aggregate since the last such start) with the usual operator
//   (f1, a1) ⊕ (f2, a2) = (f1 | f2, f2 ? a2 : a1 · a2),
// which is associative for every associative · — so it is scanned like the plain sums of ah_scan.hip, reduce-then-scan in three
// launches and for the reasons recorded there (a look-back's cross-XCD round trips on every tile's critical path, the
// co-residency deadlock, float results that depend on timing):
//   1. window_sums_kernel    one pair per tile and one per kSuper tiles             (reads the flags, the order and the column)
//   2. window_prefix_kernel  exclusive aggregates of the super pairs, one workgroup (tiny)
//   3. window_scan_kernel    the in-tile scan behind its prefix → out[order[p]]     (reads them again, one store per row)
// No workgroup ever waits for another one, and the combination tree is a function of n and the flags alone: float sums are the
// same bytes on every run.
//
// In a tile a lane holds VPT vectors of V = 2 consecutive positions (vector k of lane l: positions chunk + (k·64 + l)·2 …), so
// the order is read 16 bytes per lane, coalesced, and the flags 2 bytes per lane.  A wave scans its VPT rows of 64 vector pairs
// with shuffles; the segment start a lane sees comes from one ballot of the vectors' flags, so only the aggregates are shuffled
// and a lane takes its neighbour's value exactly when that neighbour lies at or behind the start.  ONE LDS exchange of the four
// wave pairs finishes the tile.  The gather values[order[p]] and the scatter out[order[p]] are random 1–8-byte accesses and are
// the cost of the whole thing; nothing else is written — no sorted copy of the column, no un-permute pass.
//
// The three ranking functions are the same scan over integers made of the flags: row_number and rank are a running maximum of
// {position of the last partition start, position of the last peer start} (two 32-bit halves of one word, no restarts) —
// row_number = p − partition start + 1, rank = peer start − partition start + 1 — and dense_rank is the segmented sum of bit 1.
#include <limits>
#include <type_traits>
#include "ah_common.h"
#include "ah_bytes.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int V = 2;     // consecutive positions per lane and vector: 16 bytes of the order
constexpr int VPT = 4;   // vectors per lane and tile
constexpr int WCHUNK = 64 * VPT * V;
constexpr int TILE = 2048;   // positions per tile
static_assert(TILE == kWaves * WCHUNK, "a tile is four wave chunks");
constexpr int kSuper = 8;    // tiles per workgroup in the sums pass = tile pairs a scan workgroup adds in front of its tile
constexpr int kPrefixBlock = 1024;
constexpr int kMaxOrderKeys = 8;

typedef unsigned long long u64;

// ---- the scanned operations ---------------------------------------------------------------------------------------------------
// An Op names its accumulator A, the identity and the associative combine(earlier, later), and per position
//   leaf(p, row, flag byte, &a) → bit 0: a segment starts at p, bit 1: the row's value is valid (emit writes payload 0 otherwise)
//   emit(p, row, inclusive aggregate, valid)   the ONE store of the row.
constexpr unsigned kLeafStart = 1u, kLeafValid = 2u, kLeafLive = 4u;   // (live: load_chunk's own bit — the position has a row)
constexpr u64 kQuietNaN64 = 0x7FF8000000000000ull;
constexpr unsigned kQuietNaN32 = 0x7FC00000u;

template <typename T>
struct SumOp {   // wrapping 64-bit sums of the integers (sign-extended: wraparound commutes with the widening), double for floats
  using A = typename std::conditional<std::is_floating_point<T>::value, double, u64>::type;
  const T* values;
  const uint8_t* valid;
  int64_t off;
  A* out;
  static __device__ __forceinline__ A identity() { return (A)0; }
  static __device__ __forceinline__ A combine(A x, A y) { return x + y; }
  __device__ __forceinline__ unsigned leaf(int64_t, u64 row, unsigned flag, A& a) const {
    const bool ok = ah_bit(valid, off + (int64_t)row);
    if (!ok) a = (A)0;
    else if constexpr (std::is_floating_point<T>::value) a = (double)values[row];
    else if constexpr (std::is_signed<T>::value) a = (u64)(long long)values[row];
    else a = (u64)values[row];
    return (flag & 1u) | (ok ? kLeafValid : 0u);
  }
  __device__ __forceinline__ void emit(int64_t, u64 row, A run, bool ok) const { out[row] = ok ? run : (A)0; }
};

struct CountOp {   // valid values so far; n ≤ 2^30, so 32 bits carry it
  using A = unsigned;
  const uint8_t* valid;
  int64_t off;
  long long* out;
  static __device__ __forceinline__ A identity() { return 0u; }
  static __device__ __forceinline__ A combine(A x, A y) { return x + y; }
  __device__ __forceinline__ unsigned leaf(int64_t, u64 row, unsigned flag, A& a) const {
    a = ah_bit(valid, off + (int64_t)row) ? 1u : 0u;
    return (flag & 1u) | kLeafValid;
  }
  __device__ __forceinline__ void emit(int64_t, u64 row, A run, bool) const { out[row] = (long long)run; }
};

// Minimum / maximum with the rules of ah_group_min_max_typed on the prefix.  Integers compare as themselves (widened to 32 or 64
// bits for the shuffles).  Floats compare as ordered words: the sign-magnitude → unsigned map that puts −0 below +0, with two words
// outside the range of every value for "nothing yet" (the identity) and "only NaNs so far", placed so that any value beats a NaN
// and a NaN beats nothing:  MIN: identity = ~0, NaN = ~0 − 1;  MAX: identity = 0, NaN = 1.
template <typename T, bool IS_MAX>
struct MinMaxOp {
  static constexpr bool kFloat = std::is_floating_point<T>::value;
  using W = typename std::conditional<sizeof(T) == 8, u64, unsigned>::type;                       // floats: the ordered word
  using I = typename std::conditional<sizeof(T) == 8, typename std::conditional<std::is_signed<T>::value, long long, u64>::type,
                                      typename std::conditional<std::is_signed<T>::value, int, unsigned>::type>::type;
  using A = typename std::conditional<kFloat, W, I>::type;
  const T* values;
  const uint8_t* valid;
  int64_t off;
  T* out;
  static constexpr W kSign = (W)1 << (sizeof(W) * 8 - 1);
  static constexpr W kNaNWord = IS_MAX ? (W)1 : (W)(~(W)0 - 1);
  static __device__ __forceinline__ A identity() {
    if constexpr (kFloat) return IS_MAX ? (W)0 : ~(W)0;
    else return IS_MAX ? std::numeric_limits<A>::lowest() : std::numeric_limits<A>::max();
  }
  static __device__ __forceinline__ A combine(A x, A y) { return IS_MAX ? (x > y ? x : y) : (x < y ? x : y); }
  __device__ __forceinline__ unsigned leaf(int64_t, u64 row, unsigned flag, A& a) const {
    const bool ok = ah_bit(valid, off + (int64_t)row);
    if (!ok) a = identity();
    else if constexpr (kFloat) {
      const T x = values[row];
      const W b = __builtin_bit_cast(W, x);
      a = x != x ? kNaNWord : ((b & kSign) ? ~b : (b | kSign));
    } else a = (A)values[row];
    return (flag & 1u) | (ok ? kLeafValid : 0u);
  }
  __device__ __forceinline__ void emit(int64_t, u64 row, A run, bool ok) const {
    T r;
    if constexpr (kFloat) {
      W b = (run & kSign) ? (run ^ kSign) : ~run;
      if (run == kNaNWord || run == identity()) b = sizeof(T) == 8 ? (W)kQuietNaN64 : (W)kQuietNaN32;   // the canonical quiet NaN
      if (!ok) b = 0;
      r = __builtin_bit_cast(T, b);
    } else r = ok ? (T)run : (T)0;
    out[row] = r;
  }
};

// row_number and rank: the running maximum of {last partition start : 32 | last peer start : 32} — a partition start is a peer
// start, so the low half never falls behind the high half; no restarts.  dense_rank: the sum of bit 1 restarting at bit 0.
struct StartsOp {
  using A = u64;
  int kind;
  u64* out;
  static __device__ __forceinline__ A identity() { return 0ull; }
  static __device__ __forceinline__ A combine(A x, A y) {
    const u64 hx = x >> 32, hy = y >> 32, lx = x & 0xFFFFFFFFull, ly = y & 0xFFFFFFFFull;
    return ((hx > hy ? hx : hy) << 32) | (lx > ly ? lx : ly);
  }
  __device__ __forceinline__ unsigned leaf(int64_t p, u64, unsigned flag, A& a) const {
    a = ((flag & 1u) ? ((u64)p << 32) | (u64)p : 0ull) | ((flag & 2u) ? (u64)p : 0ull);
    return kLeafValid;
  }
  __device__ __forceinline__ void emit(int64_t p, u64 row, A run, bool) const {
    const u64 part = run >> 32, peer = run & 0xFFFFFFFFull;
    out[row] = (kind == AH_WINDOW_ROW_NUMBER ? (u64)p : peer) - part + 1;
  }
};
struct DenseOp {
  using A = unsigned;
  u64* out;
  static __device__ __forceinline__ A identity() { return 0u; }
  static __device__ __forceinline__ A combine(A x, A y) { return x + y; }
  __device__ __forceinline__ unsigned leaf(int64_t, u64, unsigned flag, A& a) const {
    a = (flag & 3u) ? 1u : 0u;
    return (flag & 1u) | kLeafValid;
  }
  __device__ __forceinline__ void emit(int64_t, u64 row, A run, bool) const { out[row] = (u64)run; }
};

// ---- the shared in-tile scan ----------------------------------------------------------------------------------------------------
// What a lane holds of one wave chunk: its positions' rows, leaves and leaf bits, and after wave_rows() per vector row k the
// inclusive aggregate `inc[k]` of the row's vectors from the segment start the lane sees (or from lane 0) through its own, with
// `mask[k]` the ballot of the vectors that hold a start.
template <class Op>
struct Chunk {
  using A = typename Op::A;
  u64 row[VPT][V];
  A a[VPT][V];
  unsigned bits[VPT][V];   // kLeafStart | kLeafValid | kLeafLive; 0 for a position at or beyond n (or a row outside [0, n): never stored to)
  A inc[VPT];
  u64 mask[VPT];
};

template <class Op>
__device__ __forceinline__ void load_chunk(const Op& op, const uint8_t* __restrict__ flags, const u64* __restrict__ order, int64_t n,
                                           int64_t wbase, int lane, Chunk<Op>& c) {
#pragma unroll
  for (int k = 0; k < VPT; k++) {
    const int64_t p0 = wbase + ((int64_t)k * 64 + lane) * V;
    unsigned fl[V];
    if (p0 + V <= n) {
      unsigned short h;
      __builtin_memcpy(&h, flags + p0, 2);
      fl[0] = h & 0xFFu;
      fl[1] = h >> 8;
      if (order) {
        const ah_vec16<u64> o = ah_ld16<u64>(order + p0);
        c.row[k][0] = o.v[0];
        c.row[k][1] = o.v[1];
      } else {
        c.row[k][0] = (u64)p0;
        c.row[k][1] = (u64)p0 + 1;
      }
    } else {
#pragma unroll
      for (int j = 0; j < V; j++) {
        const bool in = p0 + j < n;
        fl[j] = in ? flags[p0 + j] : 0u;
        c.row[k][j] = in ? (order ? order[p0 + j] : (u64)(p0 + j)) : ~0ull;
      }
    }
#pragma unroll
    for (int j = 0; j < V; j++) {
      typename Op::A a = Op::identity();
      unsigned bits = 0u;
      if (c.row[k][j] < (u64)n) bits = op.leaf(p0 + j, c.row[k][j], fl[j], a) | kLeafLive;   // an order entry outside [0, n) touches nothing
      c.a[k][j] = a;
      c.bits[k][j] = bits;
    }
  }
}

template <class Op>
__device__ __forceinline__ void wave_rows(Chunk<Op>& c, int lane) {
  using A = typename Op::A;
#pragma unroll
  for (int k = 0; k < VPT; k++) {   // the vector's own pair: (a start in it, the aggregate since its last start)
    c.inc[k] = (c.bits[k][1] & kLeafStart) ? c.a[k][1] : Op::combine(c.a[k][0], c.a[k][1]);
    c.mask[k] = __ballot(((c.bits[k][0] | c.bits[k][1]) & kLeafStart) != 0u);
  }
  const u64 upto = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  int first[VPT];   // the lane of the start this lane sees in row k (none: lane 0)
#pragma unroll
  for (int k = 0; k < VPT; k++) {
    const u64 m = c.mask[k] & upto;
    first[k] = m ? 63 - __clzll((long long)m) : 0;
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
    for (int k = 0; k < VPT; k++) {
      const A t = __shfl_up(c.inc[k], o, 64);
      if (lane - o >= first[k]) c.inc[k] = Op::combine(t, c.inc[k]);
    }
  }
}

// the wave chunk's pair, folded over its VPT rows in order (the same in every lane)
template <class Op>
__device__ __forceinline__ void wave_total(const Chunk<Op>& c, bool& f, typename Op::A& a) {
  using A = typename Op::A;
  f = false;
  a = Op::identity();
#pragma unroll
  for (int k = 0; k < VPT; k++) {
    const A t = __shfl(c.inc[k], 63, 64);
    a = c.mask[k] ? t : Op::combine(a, t);
    f = f || c.mask[k] != 0ull;
  }
}

// 1. one pair per tile, one per super tile: a workgroup walks kSuper consecutive tiles, one barrier at the end
template <class Op>
__global__ __launch_bounds__(kBlock) void window_sums_kernel(Op op, const uint8_t* __restrict__ flags, const u64* __restrict__ order, int64_t n,
                                                              int64_t ntiles, typename Op::A* __restrict__ tile_a, unsigned* __restrict__ tile_f,
                                                              typename Op::A* __restrict__ super_a, unsigned* __restrict__ super_f) {
  using A = typename Op::A;
  __shared__ A s_a[kSuper][kWaves];
  __shared__ unsigned s_f[kSuper][kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t t0 = (int64_t)blockIdx.x * kSuper;
  for (int s = 0; s < kSuper; s++) {
    const int64_t tile = t0 + s;
    if (tile >= ntiles) break;
    Chunk<Op> c;
    load_chunk(op, flags, order, n, tile * TILE + (int64_t)wave * WCHUNK, lane, c);
    wave_rows(c, lane);
    bool f;
    A a;
    wave_total(c, f, a);
    if (lane == 0) { s_a[s][wave] = a; s_f[s][wave] = f ? 1u : 0u; }
  }
  __syncthreads();
  if (threadIdx.x < 64) {   // lanes 0 … kSuper − 1 fold their tile's wave pairs; their fold, in tile order, is the super pair
    A t = Op::identity();
    unsigned tf = 0u;
    if (threadIdx.x < kSuper && t0 + threadIdx.x < ntiles) {
#pragma unroll
      for (int w = 0; w < kWaves; w++) {
        t = s_f[threadIdx.x][w] ? s_a[threadIdx.x][w] : Op::combine(t, s_a[threadIdx.x][w]);
        tf |= s_f[threadIdx.x][w];
      }
      tile_a[t0 + threadIdx.x] = t;
      tile_f[t0 + threadIdx.x] = tf;
    }
    A sa = Op::identity();
    unsigned sf = 0u;
#pragma unroll
    for (int k = 0; k < kSuper; k++) {   // (a tile beyond the last one holds the identity without a start: it changes nothing)
      const A tk = __shfl(t, k, 64);
      const unsigned fk = __shfl(tf, k, 64);
      sa = fk ? tk : Op::combine(sa, tk);
      sf |= fk;
    }
    if (threadIdx.x == 0) { super_a[blockIdx.x] = sa; super_f[blockIdx.x] = sf; }
  }
}

// 2. the aggregate in front of every super tile (since the last start before it, or since position 0): one workgroup, each
// thread a contiguous run of super pairs
template <class Op>
__global__ __launch_bounds__(kPrefixBlock) void window_prefix_kernel(const typename Op::A* __restrict__ super_a, const unsigned* __restrict__ super_f,
                                                                      typename Op::A* __restrict__ super_excl, int64_t nsuper) {
  using A = typename Op::A;
  __shared__ A s_a[kPrefixBlock / 64];
  __shared__ unsigned s_f[kPrefixBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t per = (nsuper + kPrefixBlock - 1) / kPrefixBlock;
  const int64_t lo = (int64_t)threadIdx.x * per;
  const int64_t hi = lo + per < nsuper ? lo + per : nsuper;
  A a = Op::identity();
  unsigned f = 0u;
  for (int64_t q = lo; q < hi; q++) {
    a = super_f[q] ? super_a[q] : Op::combine(a, super_a[q]);
    f |= super_f[q];
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const A ta = __shfl_up(a, o, 64);
    const unsigned tf = __shfl_up(f, o, 64);
    if (lane >= o) {
      if (!f) a = Op::combine(ta, a);
      f |= tf;
    }
  }
  if (lane == 63) { s_a[wave] = a; s_f[wave] = f; }
  __syncthreads();
  A run = Op::identity();   // the waves in front, then the lanes in front
  for (int w = 0; w < wave; w++) run = s_f[w] ? s_a[w] : Op::combine(run, s_a[w]);
  const A pa = __shfl_up(a, 1, 64);
  const unsigned pf = __shfl_up(f, 1, 64);
  if (lane > 0) run = pf ? pa : Op::combine(run, pa);
  for (int64_t q = lo; q < hi; q++) {
    super_excl[q] = run;
    run = super_f[q] ? super_a[q] : Op::combine(run, super_a[q]);
  }
}

// 3. the in-tile scan behind the tile's prefix (the super prefix and the ≤ kSuper − 1 tile pairs in front of this tile in its
// super tile: workgroup-uniform loads); super_excl == nullptr: a single tile
template <class Op>
__global__ __launch_bounds__(kBlock) void window_scan_kernel(Op op, const uint8_t* __restrict__ flags, const u64* __restrict__ order, int64_t n,
                                                              const typename Op::A* __restrict__ super_excl, const typename Op::A* __restrict__ tile_a,
                                                              const unsigned* __restrict__ tile_f) {
  using A = typename Op::A;
  __shared__ A s_a[kWaves];
  __shared__ unsigned s_f[kWaves];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  const int64_t wb = tile * TILE + (int64_t)wave * WCHUNK;
  Chunk<Op> c;
  load_chunk(op, flags, order, n, wb, lane, c);
  A before = Op::identity();   // in front of the tile
  if (super_excl) {
    const int64_t sup = tile / kSuper;
    const int in_super = (int)(tile - sup * kSuper);
    before = super_excl[sup];
    for (int k = 0; k < in_super; k++) before = tile_f[sup * kSuper + k] ? tile_a[sup * kSuper + k] : Op::combine(before, tile_a[sup * kSuper + k]);
  }
  wave_rows(c, lane);
  // in front of this lane's vector k within the wave chunk: the rows before k, then the lanes before this one in row k
  bool pre_f[VPT];
  A pre_a[VPT];
  bool cf = false;
  A ca = Op::identity();
  const u64 below = (1ull << lane) - 1ull;
#pragma unroll
  for (int k = 0; k < VPT; k++) {
    A ea = __shfl_up(c.inc[k], 1, 64);
    if (lane == 0) ea = Op::identity();
    const bool ef = (c.mask[k] & below) != 0ull;
    pre_f[k] = cf || ef;
    pre_a[k] = ef ? ea : Op::combine(ca, ea);
    const A t = __shfl(c.inc[k], 63, 64);
    ca = c.mask[k] ? t : Op::combine(ca, t);
    cf = cf || c.mask[k] != 0ull;
  }
  if (lane == 0) { s_a[wave] = ca; s_f[wave] = cf ? 1u : 0u; }
  __syncthreads();
  A wa = before;   // in front of this wave chunk, the tile's prefix included
#pragma unroll
  for (int w = 0; w < kWaves; w++)
    if (w < wave) wa = s_f[w] ? s_a[w] : Op::combine(wa, s_a[w]);
#pragma unroll
  for (int k = 0; k < VPT; k++) {
    const int64_t p0 = wb + ((int64_t)k * 64 + lane) * V;
    A run = pre_f[k] ? pre_a[k] : Op::combine(wa, pre_a[k]);
#pragma unroll
    for (int j = 0; j < V; j++) {
      run = (c.bits[k][j] & kLeafStart) ? c.a[k][j] : Op::combine(run, c.a[k][j]);
      if (c.bits[k][j] & kLeafLive) op.emit(p0 + j, c.row[k][j], run, (c.bits[k][j] & kLeafValid) != 0u);
    }
  }
}

template <class Op>
int run_window(ah_ctx* c, const Op& op, const uint8_t* flags, const uint64_t* order, int64_t n) {
  using A = typename Op::A;
  const int64_t ntiles = ah_ceil_div(n, TILE);
  const u64* ord = (const u64*)order;
  if (ntiles == 1) {
    window_scan_kernel<Op><<<1, kBlock, 0, c->stream>>>(op, flags, ord, n, nullptr, nullptr, nullptr);
    AH_LAUNCH_CHECK(c);
    return AH_OK;
  }
  const int64_t nsuper = ah_ceil_div(ntiles, kSuper);
  A *tile_a = nullptr, *super_a = nullptr, *super_excl = nullptr;
  unsigned *tile_f = nullptr, *super_f = nullptr;
  auto carve = [&](TempCarver& t) {
    t.take(tile_a, (size_t)ntiles);
    t.take(tile_f, (size_t)ntiles);
    t.take(super_a, (size_t)nsuper);
    t.take(super_f, (size_t)nsuper);
    t.take(super_excl, (size_t)nsuper);
  };
  TempCarver measure;
  carve(measure);
  TempCarver block;
  int rc = ah_scratch_reserve(c, measure.used, (void**)&block.base);
  if (rc != AH_OK) return rc;
  carve(block);
  window_sums_kernel<Op><<<(unsigned)nsuper, kBlock, 0, c->stream>>>(op, flags, ord, n, ntiles, tile_a, tile_f, super_a, super_f);
  AH_LAUNCH_CHECK(c);
  window_prefix_kernel<Op><<<1, kPrefixBlock, 0, c->stream>>>(super_a, super_f, super_excl, nsuper);
  AH_LAUNCH_CHECK(c);
  window_scan_kernel<Op><<<(unsigned)ntiles, kBlock, 0, c->stream>>>(op, flags, ord, n, super_excl, tile_a, tile_f);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

// ---- the flags ----------------------------------------------------------------------------------------------------------------
struct FlagKey {   // one order key as the kernel reads it: numeric (ow = −1, rows.w = the width, values from element 0) or byte rows (ah_bytes.h, from row 0 of the call)
  ByteRows rows;
  const uint8_t* valid;
  int64_t off;
  int ow;
  int is_float;
};
struct FlagKeys {
  FlagKey k[kMaxOrderKeys];
  int n;
};

// do rows r0 and r1 tie on this key, as the sort's comparator ties them?  Both null; both NaN; equal values (−0.0 = +0.0); equal
// bytes (a decimal's value is its bytes)
__device__ __forceinline__ bool key_ties(const FlagKey& k, int64_t r0, int64_t r1) {
  const int v0 = ah_bit(k.valid, k.off + r0), v1 = ah_bit(k.valid, k.off + r1);
  if (!v0 || !v1) return v0 == v1;
  if (k.ow < 0) {
    const uint8_t* base = k.rows.data;   // the values, element `off` first
    switch (k.rows.w) {
      case 1: return base[k.off + r0] == base[k.off + r1];
      case 2: return ((const uint16_t*)base)[k.off + r0] == ((const uint16_t*)base)[k.off + r1];
      case 4:
        if (k.is_float) {
          const float x = ((const float*)base)[k.off + r0], y = ((const float*)base)[k.off + r1];
          return (x != x && y != y) || x == y;
        }
        return ((const uint32_t*)base)[k.off + r0] == ((const uint32_t*)base)[k.off + r1];
      default:
        if (k.is_float) {
          const double x = ((const double*)base)[k.off + r0], y = ((const double*)base)[k.off + r1];
          return (x != x && y != y) || x == y;
        }
        return ((const uint64_t*)base)[k.off + r0] == ((const uint64_t*)base)[k.off + r1];
    }
  }
  const uint8_t *a, *b;
  int64_t la, lb;
  row_at(k.ow, k.rows, r0, &a, &la);
  row_at(k.ow, k.rows, r1, &b, &lb);
  return la == lb && equal_bytes(a, b, la);
}

__global__ __launch_bounds__(kBlock) void window_flags_kernel(const int32_t* __restrict__ part_ids, FlagKeys keys, const u64* __restrict__ order,
                                                               int64_t n, uint8_t* __restrict__ out_flags) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x; p < n; p += stride) {
    unsigned f = 3u;
    if (p > 0) {
      const u64 r0 = order ? order[p - 1] : (u64)(p - 1), r1 = order ? order[p] : (u64)p;
      if (r0 < (u64)n && r1 < (u64)n) {   // (an order entry outside [0, n) reads nothing: it starts a partition)
        const bool part = part_ids && part_ids[r0] != part_ids[r1];
        bool peer = part || keys.n == 0;   // no order: every row is its own peer group
        for (int k = 0; k < keys.n && !peer; k++) peer = !key_ties(keys.k[k], (int64_t)r0, (int64_t)r1);
        f = (part ? 1u : 0u) | (peer ? 2u : 0u);
      }
    }
    out_flags[p] = (uint8_t)f;
  }
}

constexpr int64_t kMaxRows = (int64_t)1 << 30;

int check_common(ah_ctx* c, const char* fn, int64_t n, const void* flags, const void* out) {
  if (n < 0) return ah_fail(c, AH_EINVALID, "%s: negative length", fn);
  if (n > kMaxRows) return ah_fail(c, AH_EINVALID, "%s: %lld rows, more than 2^30", fn, (long long)n);
  if (n > 0 && (!flags || !out)) return ah_fail(c, AH_EINVALID, "%s: null buffer", fn);
  return AH_OK;
}

}  // namespace

AH_EXPORT int ah_window_flags(ah_ctx* c, const int32_t* part_ids, int nkeys, const ah_sort_key* order_keys, const uint64_t* order, int64_t n,
                              uint8_t* out_flags) {
  AH_ENTER(c);
  if (n < 0) return ah_fail(c, AH_EINVALID, "window_flags: negative length");
  if (n > kMaxRows) return ah_fail(c, AH_EINVALID, "window_flags: %lld rows, more than 2^30", (long long)n);
  if (nkeys < 0 || nkeys > kMaxOrderKeys) return ah_fail(c, AH_EINVALID, "window_flags: %d order keys, more than %d", nkeys, kMaxOrderKeys);
  if (nkeys > 0 && !order_keys) return ah_fail(c, AH_EINVALID, "window_flags: null key table");
  if (n == 0) return AH_OK;
  if (!out_flags) return ah_fail(c, AH_EINVALID, "window_flags: null buffer");
  FlagKeys keys{};
  keys.n = nkeys;
  for (int i = 0; i < nkeys; i++) {
    const ah_sort_key& s = order_keys[i];
    FlagKey& k = keys.k[i];
    if (s.off < 0) return ah_fail(c, AH_EINVALID, "window_flags: key %d has a negative offset", i);
    k.valid = s.valid;
    k.off = s.off;
    const int w = ah_type_width(s.type);
    if (w) {
      if (!s.values) return ah_fail(c, AH_EINVALID, "window_flags: key %d has no values", i);
      if ((uintptr_t)s.values & (uintptr_t)(w - 1)) return ah_fail(c, AH_EINVALID, "window_flags: key %d is not element-aligned", i);
      k.ow = -1;
      k.is_float = s.type == AH_FLOAT32 || s.type == AH_FLOAT64;
      k.rows = ByteRows{nullptr, (const uint8_t*)s.values, w};
    } else if (s.type == AH_BINARY || s.type == AH_LARGE_BINARY) {
      if (!s.offsets) return ah_fail(c, AH_EINVALID, "window_flags: key %d has no offsets", i);
      k.ow = s.type == AH_BINARY ? 4 : 8;
      k.rows = byte_rows(k.ow, s.offsets, (const uint8_t*)s.values, 0, s.off);   // the offsets of entry `off`: row r is entry r
    } else if (s.type == AH_FIXED_SIZE_BINARY || s.type == AH_DECIMAL128 || s.type == AH_DECIMAL256) {
      const int bw = s.type == AH_DECIMAL128 ? 16 : s.type == AH_DECIMAL256 ? 32 : s.byte_width;
      if (bw < 0 || bw > 4096) return ah_fail(c, AH_EINVALID, "window_flags: key %d has byte width %d", i, bw);
      if (bw > 0 && !s.values) return ah_fail(c, AH_EINVALID, "window_flags: key %d has no values", i);
      k.ow = 0;
      k.rows = byte_rows(0, nullptr, (const uint8_t*)s.values, bw, s.off);   // slot `off` first: row r is slot r
    } else {
      return ah_fail(c, AH_ENOTIMPL, "window_flags: key %d has type %d, which sort_indices does not order", i, s.type);
    }
  }
  window_flags_kernel<<<ah_stream_grid(c, ah_ceil_div(n, kBlock), 8), kBlock, 0, c->stream>>>(part_ids, keys, (const u64*)order, n, out_flags);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

AH_EXPORT int ah_window_rank(ah_ctx* c, int kind, const uint8_t* flags, const uint64_t* order, int64_t n, uint64_t* out) {
  AH_ENTER(c);
  int rc = check_common(c, "window_rank", n, flags, out);
  if (rc != AH_OK) return rc;
  if (kind != AH_WINDOW_ROW_NUMBER && kind != AH_WINDOW_RANK && kind != AH_WINDOW_DENSE_RANK)
    return ah_fail(c, AH_EINVALID, "window_rank: unknown kind %d", kind);
  if (n == 0) return AH_OK;
  if (kind == AH_WINDOW_DENSE_RANK) return run_window(c, DenseOp{(u64*)out}, flags, order, n);
  return run_window(c, StartsOp{kind, (u64*)out}, flags, order, n);
}

AH_EXPORT int ah_window_scan(ah_ctx* c, int op, int type, const void* values, const uint8_t* valid, int64_t off, const uint8_t* flags,
                             const uint64_t* order, int64_t n, void* out_values) {
  AH_ENTER(c);
  int rc = check_common(c, "window_scan", n, flags, out_values);
  if (rc != AH_OK) return rc;
  if (off < 0) return ah_fail(c, AH_EINVALID, "window_scan: negative offset");
  if (op != AH_WINDOW_SUM && op != AH_WINDOW_MIN && op != AH_WINDOW_MAX && op != AH_WINDOW_COUNT)
    return ah_fail(c, AH_EINVALID, "window_scan: unknown op %d", op);
  if (op == AH_WINDOW_COUNT) {   // reads the validity bits only
    if (n == 0) return AH_OK;
    if ((uintptr_t)out_values & 7) return ah_fail(c, AH_EINVALID, "window_scan: output not element-aligned");
    return run_window(c, CountOp{valid, off, (long long*)out_values}, flags, order, n);
  }
  const int w = ah_type_width(type);
  if (!w) return ah_fail(c, AH_ENOTIMPL, "window_scan: value type %d is not numeric", type);
  if (n == 0) return AH_OK;
  if (!values) return ah_fail(c, AH_EINVALID, "window_scan: null buffer");
  const int ow = op == AH_WINDOW_SUM ? 8 : w;
  if (((uintptr_t)values & (uintptr_t)(w - 1)) || ((uintptr_t)out_values & (uintptr_t)(ow - 1)))
    return ah_fail(c, AH_EINVALID, "window_scan: buffer not element-aligned");
  rc = AH_OK;
  with_numeric_type(type, [&](auto t) {
    using T = typename decltype(t)::type;
    if (op == AH_WINDOW_SUM) rc = run_window(c, SumOp<T>{(const T*)values, valid, off, (typename SumOp<T>::A*)out_values}, flags, order, n);
    else if (op == AH_WINDOW_MIN) rc = run_window(c, MinMaxOp<T, false>{(const T*)values, valid, off, (T*)out_values}, flags, order, n);
    else rc = run_window(c, MinMaxOp<T, true>{(const T*)values, valid, off, (T*)out_values}, flags, order, n);
  });
  return rc;
}
