// ah_sort_radix.h — the stable 8-bit LSD radix pass shared by the sorts (ah_sort.hip: numeric keys and the group-by
// partition; ah_sort_binary.hip: binary, fixed-size binary and decimal keys; ah_select.hip: the survivors of select_k), the
// order-preserving key and the row categories of a numeric sort key, and the temporaries of one sort_indices call.
// Everything here lives in an anonymous namespace: every translation unit that includes it gets its own instances.
#pragma once
#include <algorithm>
#include <type_traits>
#include <vector>
#include "ah_common.h"
#include "ah_reduce.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kItems = 8;                       // rounds of 64 rows per wave per tile
constexpr int kTile = kBlock * kItems;          // 2048 rows
constexpr int kRadix = 256;
constexpr int kAndOrGrid = 4096;                 // most workgroups the two key-reduction kernels are launched with (their partials live in SortBuffers::andor)
constexpr int kMaxTilesPerBlock = 8;             // tiles one workgroup handles = granularity of the histogram / scan

// small inputs keep one tile per workgroup (parallelism), large ones eight (fewer histogram rows)
static inline int tiles_per_block(int64_t n) { return n >= ((int64_t)1 << 24) ? kMaxTilesPerBlock : 1; }

// the three categories of a sort key's rows and the key transform: shared by the sort (ah_sort.hip) and select_k (ah_select.hip)
enum { kCatRest = 0, kCatNaN = 1, kCatNull = 2 };

// order-preserving unsigned key, zero-extended to 64 bits
template <typename T>
__device__ __forceinline__ unsigned long long make_key(T v, bool descending) {
  using U = typename std::make_unsigned<typename std::conditional<std::is_floating_point<T>::value,
                                                                    typename std::conditional<sizeof(T) == 4, int, long long>::type, T>::type>::type;
  constexpr U sign = (U)1 << (sizeof(T) * 8 - 1);
  U k;
  if constexpr (std::is_floating_point<T>::value) {
    if (v == (T)0) v = (T)0;  // −0.0 → +0.0: they tie (cmp.Compare)
    U b = __builtin_bit_cast(U, v);
    k = (b & sign) ? (U)~b : (U)(b | sign);
  } else if constexpr (std::is_signed<T>::value) {
    k = (U)v ^ sign;
  } else {
    k = (U)v;
  }
  if (descending) k = (U)~k;
  return (unsigned long long)k;
}

struct Pairs {
  const unsigned long long* keys;
  const unsigned* rows;
  int shift;
  __device__ __forceinline__ void load(int64_t i, unsigned long long* key, unsigned* row, unsigned* digit) const {
    *key = keys[i];
    *row = rows[i];
    *digit = (unsigned)(*key >> shift) & 255u;
  }
};

// block histogram → hist[digit * nblocks + block]; a block = 1 or 8 consecutive tiles handled by one
// workgroup (one histogram row per 16 Ki rows: 8× fewer scattered 4-byte writes and an 8× smaller scan)
template <typename SRC>
__global__ __launch_bounds__(kBlock) void hist_kernel(SRC src, int64_t n, unsigned* __restrict__ hist, int64_t nblocks, int tpb) {
  __shared__ unsigned s_h[kWaves][kRadix];
  for (int i = threadIdx.x; i < kWaves * kRadix; i += kBlock) (&s_h[0][0])[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t block = blockIdx.x;
  for (int t = 0; t < tpb; t++) {
    const int64_t wbase = (block * tpb + t) * kTile + (int64_t)wave * (kItems * 64);
    if (wbase >= n) break;
#pragma unroll
    for (int r = 0; r < kItems; r++) {
      const int64_t i = wbase + r * 64 + lane;
      if (i < n) {
        unsigned long long key; unsigned row, digit;
        src.load(i, &key, &row, &digit);
        atomicAdd(&s_h[wave][digit], 1u);
      }
    }
  }
  __syncthreads();
  for (int d = threadIdx.x; d < kRadix; d += kBlock) {
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) t += s_h[w][d];
    hist[(int64_t)d * nblocks + block] = t;
  }
}

// stable scatter: offs = INCLUSIVE scan of hist (digit-major)
template <typename SRC>
__global__ __launch_bounds__(kBlock) void scatter_kernel(SRC src, int64_t n, const unsigned* __restrict__ hist, const unsigned* __restrict__ offs,
                                                          int64_t nblocks, int tpb, unsigned long long* __restrict__ out_keys,
                                                          unsigned* __restrict__ out_rows) {
  __shared__ unsigned s_cnt[kWaves][kRadix];   // per wave: rows of each digit seen in earlier rounds; later: wave bases
  __shared__ unsigned s_start[kRadix], s_goff[kRadix], s_wsum[kWaves];
  __shared__ unsigned long long s_keys[kTile];
  __shared__ unsigned s_rows[kTile];
  __shared__ uint8_t s_dig[kTile];
  static_assert(kBlock == kRadix, "one thread per digit in the prefix step");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // thread d carries the global position of the block's next row of digit d (inclusive scan − own count)
  unsigned run_d = offs[(int64_t)threadIdx.x * nblocks + blockIdx.x] - hist[(int64_t)threadIdx.x * nblocks + blockIdx.x];
  for (int tb = 0; tb < tpb; tb++) {
  const int64_t tile = (int64_t)blockIdx.x * tpb + tb;
  if (tile * kTile >= n) break;  // workgroup-uniform
  for (int i = threadIdx.x; i < kWaves * kRadix; i += kBlock) (&s_cnt[0][0])[i] = 0;
  __syncthreads();
  const int64_t wbase = tile * kTile + (int64_t)wave * (kItems * 64);
  unsigned long long key[kItems];
  unsigned row[kItems], digit[kItems], rank[kItems];
  bool live[kItems];
#pragma unroll
  for (int r = 0; r < kItems; r++) {
    const int64_t i = wbase + r * 64 + lane;
    live[r] = i < n;
    key[r] = 0; row[r] = 0; digit[r] = 0;
    if (live[r]) src.load(i, &key[r], &row[r], &digit[r]);
  }
  // in-wave ranks, round by round: element order inside the tile is (wave, round, lane)
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
  for (int r = 0; r < kItems; r++) {
    // match-any on the 8-bit digit: peers = lanes holding the same digit
    unsigned long long peers = __ballot(live[r]);
#pragma unroll
    for (int b = 0; b < 8; b++) {
      const unsigned long long bal = __ballot((digit[r] >> b) & 1u);
      peers &= ((digit[r] >> b) & 1u) ? bal : ~bal;
    }
    if (live[r]) {
      // atomic accesses: ANOTHER lane of this wave advanced the counter in the previous round — a value
      // the per-thread memory model would otherwise let the compiler keep in a register
      unsigned* cnt = &s_cnt[wave][digit[r]];
      const unsigned before = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);  // every peer reads the same counter …
      rank[r] = before + (unsigned)__popcll(peers & below);
      if ((peers & below) == 0)  // … the lowest one advances it
        __hip_atomic_store(cnt, before + (unsigned)__popcll(peers), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    // LDS operations of one wave execute in order; keep the compiler from moving them across rounds
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  // per digit: exclusive prefix over the waves, the digit's start inside the tile (exclusive scan over
  // the 256 digit totals), and the offset that turns a tile-local sorted position into the global one
  unsigned tot = 0;  // thread d < 256 owns digit d (kBlock == kRadix)
  {
    const int d = threadIdx.x;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
      const unsigned t = s_cnt[w][d];
      s_cnt[w][d] = tot;
      tot += t;
    }
    unsigned inc = tot;  // inclusive scan of the digit totals: shuffles inside a wave, LDS across waves
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) s_wsum[wave] = inc;
    __syncthreads();
    unsigned wbase = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) if (w < wave) wbase += s_wsum[w];
    const unsigned start = wbase + inc - tot;                       // first tile-local position of digit d
    s_start[d] = start;
    s_goff[d] = run_d - start;     // global = s_goff[d] + local
    run_d += tot;
  }
  __syncthreads();
  // stage the tile in digit order in LDS …
#pragma unroll
  for (int r = 0; r < kItems; r++) {
    if (live[r]) {
      const unsigned lp = s_start[digit[r]] + s_cnt[wave][digit[r]] + rank[r];
      s_keys[lp] = key[r];
      s_rows[lp] = row[r];
      s_dig[lp] = (uint8_t)digit[r];
    }
  }
  __syncthreads();
  // … and write it out: consecutive threads hold consecutive positions of the same digit run, so the
  // stores to HBM are runs of neighbouring addresses instead of one 8-byte store per bucket
  const int64_t tile_n = n - tile * kTile >= kTile ? kTile : n - tile * kTile;
  for (int lp = threadIdx.x; lp < tile_n; lp += kBlock) {
    const unsigned pos = s_goff[s_dig[lp]] + (unsigned)lp;
    out_keys[pos] = s_keys[lp];
    out_rows[pos] = s_rows[lp];
  }
  }  // tiles of this block
}

// Which key bits vary at all, the extreme keys, and (pairs_kernel, ah_sort.hip) how many rows were NaN: a part of the reduction layer
// (ah_reduce.h).  Per workgroup; the host folds the ≤ 1024 partial results — same-address atomics per wave would cost more than the pass.
struct KeyStats {
  unsigned long long a, o, mn, mx, nans;
  __device__ __forceinline__ void init() { a = ~0ull; o = 0ull; mn = ~0ull; mx = 0ull; nans = 0; }
  __device__ __forceinline__ void add(unsigned long long k) { a &= k; o |= k; mn = k < mn ? k : mn; mx = k > mx ? k : mx; }
  __device__ __forceinline__ void merge(const KeyStats& p) {
    a &= p.a; o |= p.o;
    mn = p.mn < mn ? p.mn : mn;
    mx = p.mx > mx ? p.mx : mx;
    nans += p.nans;
  }
  // res[0 … NWORDS): {AND, OR, min, max} and, with NWORDS = 5, the NaN count
  template <int NWORDS>
  __device__ __forceinline__ void store(unsigned long long* res) const {
    res[0] = a; res[1] = o; res[2] = mn; res[3] = mx;
    if (NWORDS == 5) res[4] = nans;
  }
};

__global__ __launch_bounds__(kBlock) void and_or_kernel(const unsigned long long* __restrict__ keys, int64_t n, unsigned long long* __restrict__ res) {
  KeyStats st;
  st.init();
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) st.add(keys[i]);
  st = ah_block_reduce<kBlock>(st);
  if (threadIdx.x == 0) st.store<4>(res + (size_t)blockIdx.x * 4);
}

// temporaries of one call, carved out of the context's temp arena (the scratch arena is used by the scan this calls)
struct Carver {
  uint8_t* base;
  size_t used = 0;
  static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
  template <typename P>
  void take(size_t bytes, P** out) { *out = (P*)(base + used); used += pad(bytes); }
};

template <typename SRC>
int radix_pass(ah_ctx* c, SRC src, int64_t n, unsigned* hist, unsigned* offs, unsigned long long* out_keys, unsigned* out_rows) {
  const int tpb = tiles_per_block(n);
  const int64_t nblocks = ah_ceil_div(n, (int64_t)kTile * tpb);
  hist_kernel<SRC><<<(unsigned)nblocks, kBlock, 0, c->stream>>>(src, n, hist, nblocks, tpb);
  AH_LAUNCH_CHECK(c);
  int rc = ah_cumulative_sum(c, AH_UINT32, hist, nullptr, 0, (int64_t)kRadix * nblocks, nullptr, 0, 0, offs, nullptr, nullptr);
  if (rc != AH_OK) return rc;
  scatter_kernel<SRC><<<(unsigned)nblocks, kBlock, 0, c->stream>>>(src, n, hist, offs, nblocks, tpb, out_keys, out_rows);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

}  // namespace

// One sort key of a call.  Numeric: `values` is the value of row 0 of the call (as ah_sort_indices takes it).  Binary /
// large binary: offsets[off + i] .. offsets[off + i + 1] delimit row i inside `data`.  Fixed-size binary / decimal: row i is
// the `width` bytes at data + (off + i)·width.  Validity bit off + i in every case.
struct SortCol {
  int type;
  const void* values;
  const void* offsets;
  const uint8_t* data;
  int width;
  const uint8_t* valid;
  int64_t off;
  int descending, nulls_at_start;
};

constexpr int kBinArrays = 8;

struct SortBuffers {  // temporaries shared by all keys of one call
  void* msd_tmp = nullptr;  // ah_sort_msd.hip's tables (nullptr: that path is off for this call)
  uint64_t* final_out = nullptr;  // single-key call: where the widened result goes; the MSD path writes it directly when every row is `rest`
  int64_t final_n = 0;            // … and how many entries of the order go there (n, or the head select_k asks for)
  bool emitted = false;
  unsigned long long *ka, *kb, *andor;
  unsigned *ra, *rb, *rc;  // ra / rb: ping-pong of a key's passes; rc: the previous key's result
  unsigned *hist, *offs;
  unsigned* bin[kBinArrays] = {};  // binary keys only: arrays of n words (ah_sort_binary.hip); nullptr when every key is numeric
};

bool ah_sort_is_binary(int type);
// Stable sort of the current row order (rows_in, or the input order) by one binary, fixed-size binary or decimal column; the
// new order lands in b.ra — the contract of the numeric sort_by_column (ah_sort.hip).
int ah_sort_by_binary(ah_ctx* c, SortBuffers& b, const SortCol& col, int64_t n, const unsigned* rows_in);

