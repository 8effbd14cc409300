// ah_select.hip — select_k: the first k entries of sort_indices without the sort (ORDER BY … LIMIT k).
//
// The contract is the sort's (kernels.SortIndices, arrow/compute/internal/kernels/vector_sort.go:388-481; ah_sort.hip has the
// rules): ah_select_k returns exactly the first min(k, n) entries ah_sort_indices_keys returns for the same keys — stable, −0.0
// ties +0.0, NaNs next to the nulls, nulls at the end or the start.  Arrow C++ calls the function select_k_unstable; the stable
// answer given here is one of the answers it allows.
//
// AH_SELECT_SORT   the sort, with its last step (widening the row numbers into the output) cut at k entries: total over every key
//                  type the sort takes, at the cost of the sort.
// AH_SELECT_RADIX  first key numeric.  Passes over key 0 only, 1 read of the column each:
//   classify   rest / NaN / null counts and the smallest and largest rest key (KeyStats); one read-back.  From the counts and the
//              placement the host knows how many rest (k_rest), NaN and null rows the answer holds.
//   threshold  MSD histogram levels of 11 bits over nk = (key − min) << clz(max − min), so the first level always splits.  A
//              level counts the rows whose decided bits equal the prefix so far; a one-workgroup kernel picks the bin holding the
//              k_rest-th key and leaves {prefix, remaining rank, rows below} in device memory for the next level — no host round
//              trip between levels.  The levels stop when every varying bit is decided or the bin holds ≤ kSelSmallBin rows
//              (later launches see `done` and return); one read-back of the state.
//   collect    rows whose prefix is below the threshold's all belong; of the rows that share it the first take_eq in row order
//              (all of them after an early stop or with several keys; the remaining rank when the threshold is exact — so a
//              constant column costs the same passes as a random one).  A truncated stable compaction: per-tile counts of
//              {below, equal, NaN, null}, the scan (ah_cumulative_sum), a fill that reads only tiles that contribute.  The NaN
//              and null rows the answer needs are the first of their category in row order and go straight to the output.
//   order      one key: the (nk, row) pairs — two segments, each in row order, with disjoint keys — by a one-workgroup bitonic
//              network in LDS (≤ kSelRankSort pairs) or the stable LSD passes over the bytes of nk that can vary; cut at k_rest; widened.
//              several keys: the candidate rows ordered by all keys with the sort itself (ah_sort_rows_keys), cut at k_rest.
// Two cases of several keys take the sort route whatever was asked: k reaching into the NaN / null group of key 0 (the next key
// orders that group), and candidates above n / kSelCandidateShare.
#include <algorithm>
#include <vector>
#include "ah_sort_radix.h"

namespace {

constexpr int kSelLevels = 6;                  // 5 × 11 bits + 9 bits
constexpr int kSelBins = 2048;                 // bins of one level (LDS: 8 KiB per workgroup)
constexpr unsigned kSelSmallBin = 1024;        // a surviving bin this small is finished by ordering it
constexpr int kSelRankSort = 2048;             // pairs the one-workgroup bitonic network takes (a power of two)
constexpr int kSelRounds = 16;                 // rounds of 64 rows per wave per tile
constexpr int kSelTile = kBlock * kSelRounds;  // 4096 rows: the tile of the count / fill passes
constexpr int kSelStatsGrid = 1024;            // most workgroups of the classify pass
constexpr int kSelCandidateShare = 8;          // several keys: candidates above n / 8 → the sort route
constexpr int kSelUnroll = 4;

enum { kSelBelow = 0, kSelEqual = 1, kSelNaN = 2, kSelNull = 3, kSelNone = 4 };
enum { kModeThreshold = 0, kModeNoRest = 1, kModeAllRest = 2 };

__host__ __device__ constexpr int sel_level_shift(int level) { return 64 - 11 * (level + 1) > 0 ? 64 - 11 * (level + 1) : 0; }
__host__ __device__ constexpr int sel_level_bits(int level) { return level < 5 ? 11 : 9; }

// what the threshold levels hand from one to the next, and at the end to the host
struct SelState {
  unsigned long long prefix;   // the decided bits of the threshold: nk >> shift
  unsigned rank;               // 1-based rank of the wanted key among the rows sharing the prefix
  unsigned below;              // rows whose decided bits are below the prefix
  unsigned take_eq;            // rows sharing the prefix that the collect pass takes, in row order
  unsigned shift;
  unsigned done;
  unsigned pad;
};

template <typename T>
struct SelCol {
  const T* values;             // row 0 of the call
  const uint8_t* valid;
  int64_t off;
  int descending;
  unsigned long long kmin;
  int lz;
  __device__ __forceinline__ int load(int64_t i, unsigned long long* nk) const {
    const T v = values[i];
    *nk = 0;
    if (!ah_bit(valid, off + i)) return kCatNull;
    if (std::is_floating_point<T>::value && v != v) return kCatNaN;
    *nk = (make_key<T>(v, descending) - kmin) << lz;
    return kCatRest;
  }
};

struct SelStats {
  KeyStats k;
  unsigned long long nulls;
  __device__ __forceinline__ void init() { k.init(); nulls = 0; }
  __device__ __forceinline__ void merge(const SelStats& p) { k.merge(p.k); nulls += p.nulls; }
};

// classify: res[8 b …] = {min, max, NaNs, nulls} of workgroup b (raw keys: col.kmin = 0, col.lz = 0)
template <typename T>
__global__ __launch_bounds__(kBlock) void sel_classify_kernel(SelCol<T> col, int64_t n, unsigned long long* __restrict__ res) {
  SelStats st;
  st.init();
  const int64_t stride = (int64_t)gridDim.x * kBlock * kSelUnroll;
  for (int64_t base = (int64_t)blockIdx.x * kBlock * kSelUnroll; base < n; base += stride) {
#pragma unroll
    for (int u = 0; u < kSelUnroll; u++) {
      const int64_t i = base + (int64_t)u * kBlock + threadIdx.x;
      if (i >= n) continue;
      unsigned long long key;
      const int cat = col.load(i, &key);
      if (cat == kCatRest) st.k.add(key);
      else if (cat == kCatNaN) st.k.nans++;
      else st.nulls++;
    }
  }
  st = ah_block_reduce<kBlock>(st);
  if (threadIdx.x == 0) {
    unsigned long long* r = res + (size_t)blockIdx.x * 8;
    r[0] = st.k.mn; r[1] = st.k.mx; r[2] = st.k.nans; r[3] = st.nulls;
  }
}

// one level: the histogram of this level's digit over the rest rows whose decided bits equal the prefix
template <typename T>
__global__ __launch_bounds__(kBlock) void sel_hist_kernel(SelCol<T> col, int64_t n, int level, const SelState* __restrict__ st,
                                                           unsigned* __restrict__ ghist) {
  __shared__ unsigned s_h[kSelBins];
  unsigned long long prefix = 0;
  int pshift = 0;
  if (level > 0) {
    if (st->done) return;   // the same word for every thread
    prefix = st->prefix;
    pshift = (int)st->shift;
  }
  const int shift = sel_level_shift(level);
  const unsigned mask = (1u << sel_level_bits(level)) - 1u;
  for (int i = threadIdx.x; i < kSelBins; i += kBlock) s_h[i] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * kBlock * kSelUnroll;
  for (int64_t base = (int64_t)blockIdx.x * kBlock * kSelUnroll; base < n; base += stride) {   // base is workgroup-uniform
    unsigned long long nk[kSelUnroll];
    bool live[kSelUnroll];
#pragma unroll
    for (int u = 0; u < kSelUnroll; u++) {
      const int64_t i = base + (int64_t)u * kBlock + threadIdx.x;
      nk[u] = 0;
      live[u] = i < n && col.load(i, &nk[u]) == kCatRest;
    }
#pragma unroll
    for (int u = 0; u < kSelUnroll; u++) {
      const bool in = live[u] && (level == 0 || (nk[u] >> pshift) == prefix);
      const unsigned bin = (unsigned)(nk[u] >> shift) & mask;
      const unsigned long long bal = __ballot(in);
      if (bal == 0) continue;
      // a duplicate-heavy column puts the whole wave into one bin: one add for the wave instead of 64 to one LDS address
      const int first = __ffsll((long long)bal) - 1;
      const unsigned fbin = (unsigned)__shfl((int)bin, first, 64);
      if (__ballot(in && bin == fbin) == bal) {
        if (lane == first) atomicAdd(&s_h[fbin], (unsigned)__popcll(bal));
      } else if (in) {
        atomicAdd(&s_h[bin], 1u);
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kSelBins; b += kBlock) {
    const unsigned v = s_h[b];
    if (v) atomicAdd(&ghist[b], v);
  }
}

// one workgroup: the bin that holds the wanted rank; the state for the next level
__global__ __launch_bounds__(kBlock) void sel_pick_kernel(const unsigned* __restrict__ ghist, SelState* st, int level, unsigned rank0, int is_last,
                                                           int all_ties) {
  __shared__ unsigned s_wave[kWaves];
  const bool first_level = level == 0;
  const unsigned done = first_level ? 0u : st->done;
  const unsigned rank = first_level ? rank0 : st->rank;
  const unsigned below = first_level ? 0u : st->below;
  const unsigned long long prefix = first_level ? 0ull : st->prefix;
  if (done) return;
  constexpr int kPer = kSelBins / kBlock;   // 8 bins per thread; the 9-bit level leaves the upper bins zero
  unsigned h[kPer], sum = 0;
#pragma unroll
  for (int j = 0; j < kPer; j++) { h[j] = ghist[threadIdx.x * kPer + j]; sum += h[j]; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned inc = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();   // also: every thread has read the state before one of them writes it
  unsigned wbase = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) if (w < wave) wbase += s_wave[w];
  inc += wbase;
  const unsigned exc = inc - sum;
  if (exc < rank && rank <= inc) {   // one thread
    unsigned run = exc;
    int bin = 0;
    unsigned cnt = 0;
#pragma unroll
    for (int j = 0; j < kPer; j++) {
      if (cnt == 0 && rank <= run + h[j]) { bin = threadIdx.x * kPer + j; cnt = h[j]; }
      if (cnt == 0) run += h[j];
    }
    const bool fin = is_last || cnt <= kSelSmallBin;
    st->prefix = (prefix << sel_level_bits(level)) | (unsigned long long)bin;
    st->below = below + run;
    st->rank = rank - run;
    st->shift = (unsigned)sel_level_shift(level);
    st->take_eq = (is_last && !all_ties) ? rank - run : cnt;
    st->done = fin ? 1u : 0u;
  }
}

struct SelCut {
  unsigned long long prefix;
  int shift;
  int mode;
};

template <typename T>
__device__ __forceinline__ int sel_code(const SelCol<T>& col, int64_t i, const SelCut& cut, unsigned long long* nk) {
  const int cat = col.load(i, nk);
  if (cat == kCatNull) return kSelNull;
  if (cat == kCatNaN) return kSelNaN;
  if (cut.mode == kModeNoRest) return kSelNone;
  if (cut.mode == kModeAllRest) return kSelEqual;
  const unsigned long long q = *nk >> cut.shift;
  return q < cut.prefix ? kSelBelow : q == cut.prefix ? kSelEqual : kSelNone;
}

// per-tile counts of the four categories: hist4[category · ntiles + tile]
template <typename T>
__global__ __launch_bounds__(kBlock) void sel_count_kernel(SelCol<T> col, int64_t n, int64_t ntiles, SelCut cut, unsigned* __restrict__ hist4) {
  __shared__ unsigned s_w[kWaves][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  const int64_t wbase = tile * kSelTile + (int64_t)wave * (kSelRounds * 64);
  unsigned cnt[4] = {0, 0, 0, 0};
#pragma unroll 4
  for (int r = 0; r < kSelRounds; r++) {
    const int64_t i = wbase + r * 64 + lane;
    unsigned long long nk;
    const int code = i < n ? sel_code(col, i, cut, &nk) : kSelNone;
#pragma unroll
    for (int c = 0; c < 4; c++) cnt[c] += code == c;
  }
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const unsigned t = ah_wave_sum(cnt[c]);
    if (lane == 0) s_w[wave][c] = t;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned t = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) t += s_w[w][threadIdx.x];
    hist4[(int64_t)threadIdx.x * ntiles + tile] = t;
  }
}

struct SelOut {
  unsigned long long* pk;   // `below` pairs in row order, then take_eq `equal` pairs in row order
  unsigned* pr;
  uint64_t* out_nan;        // the answer's NaN rows and null rows, where they belong in the output
  uint64_t* out_null;
  unsigned below, take_eq, k_nan, k_null;
};

// the fill of the truncated stable compaction; offs4 = inclusive scan of hist4.  Element order inside a tile: (wave, round, lane).
template <typename T>
__global__ __launch_bounds__(kBlock) void sel_fill_kernel(SelCol<T> col, int64_t n, int64_t ntiles, SelCut cut, const unsigned* __restrict__ hist4,
                                                           const unsigned* __restrict__ offs4, SelOut o) {
  __shared__ unsigned s_base[4], s_need[4], s_w[kWaves][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t tile = blockIdx.x;
  if (threadIdx.x < 4) {
    const int c = threadIdx.x;
    const unsigned h = hist4[(int64_t)c * ntiles + tile];
    const unsigned start = c > 0 ? offs4[(int64_t)c * ntiles - 1] : 0u;
    const unsigned base = offs4[(int64_t)c * ntiles + tile] - h - start;   // rows of this category in earlier tiles
    const unsigned limit = c == kSelBelow ? o.below : c == kSelEqual ? o.take_eq : c == kSelNaN ? o.k_nan : o.k_null;
    s_base[c] = base;
    s_need[c] = h > 0 && base < limit;
  }
  __syncthreads();
  if (!(s_need[0] | s_need[1] | s_need[2] | s_need[3])) return;   // most tiles when k is small: nothing read
  const int64_t wbase = tile * kSelTile + (int64_t)wave * (kSelRounds * 64);
  unsigned tot[4] = {0, 0, 0, 0};
  for (int r = 0; r < kSelRounds; r++) {
    const int64_t i = wbase + r * 64 + lane;
    unsigned long long nk;
    const int code = i < n ? sel_code(col, i, cut, &nk) : kSelNone;
#pragma unroll
    for (int c = 0; c < 4; c++) tot[c] += (unsigned)__popcll(__ballot(code == c));
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 4; c++) s_w[wave][c] = tot[c];
  }
  __syncthreads();
  unsigned run[4];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    run[c] = s_base[c];
    for (int w = 0; w < kWaves; w++) if (w < wave) run[c] += s_w[w][c];
  }
  const unsigned long long lower = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int r = 0; r < kSelRounds; r++) {   // the tile's rows again: they are in the cache
    const int64_t i = wbase + r * 64 + lane;
    unsigned long long nk;
    const int code = i < n ? sel_code(col, i, cut, &nk) : kSelNone;
    unsigned rank = 0;
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const unsigned long long bal = __ballot(code == c);
      if (code == c) rank = run[c] + (unsigned)__popcll(bal & lower);
      run[c] += (unsigned)__popcll(bal);
    }
    if (code == kSelBelow) {
      if (rank < o.below) { o.pk[rank] = nk; o.pr[rank] = (unsigned)i; }
    } else if (code == kSelEqual) {
      if (rank < o.take_eq) { o.pk[o.below + rank] = nk; o.pr[o.below + rank] = (unsigned)i; }
    } else if (code == kSelNaN) {
      if (rank < o.k_nan) o.out_nan[rank] = (uint64_t)i;
    } else if (code == kSelNull) {
      if (rank < o.k_null) o.out_null[rank] = (uint64_t)i;
    }
  }
}

// ≤ kSelRankSort pairs, one workgroup: a bitonic network over (key, row) in LDS, padded to a power of two with pairs above
// every real one; the first k rows leave.  Rows are distinct, so the order is total and ties on the key come out in row order.
__global__ __launch_bounds__(kBlock) void sel_bitonic_kernel(const unsigned long long* __restrict__ pk, const unsigned* __restrict__ pr, int m, unsigned k,
                                                              uint64_t* __restrict__ out) {
  __shared__ unsigned long long s_k[kSelRankSort];
  __shared__ unsigned s_r[kSelRankSort];
  int p = 2;
  while (p < m) p <<= 1;   // ≤ kSelRankSort: the host sends no more pairs than that
  for (int i = threadIdx.x; i < p; i += kBlock) {
    s_k[i] = i < m ? pk[i] : ~0ull;
    s_r[i] = i < m ? pr[i] : ~0u;
  }
  __syncthreads();
  for (int size = 2; size <= p; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = threadIdx.x; t < (p >> 1); t += kBlock) {
        const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
        const unsigned long long ka = s_k[lo], kb = s_k[hi];
        const unsigned ra = s_r[lo], rb = s_r[hi];
        const bool above = ka > kb || (ka == kb && ra > rb);
        if (above == ((lo & size) == 0)) { s_k[lo] = kb; s_k[hi] = ka; s_r[lo] = rb; s_r[hi] = ra; }
      }
      __syncthreads();
    }
  }
  const int written = (int)k < m ? (int)k : m;
  for (int i = threadIdx.x; i < written; i += kBlock) out[i] = s_r[i];
}

__global__ __launch_bounds__(kBlock) void sel_emit_kernel(const unsigned* __restrict__ rows, int64_t k, uint64_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < k; i += stride) out[i] = rows[i];
}

// the sort route: the sort itself, its last step — widening the row numbers into the output — cut at kk entries
int select_by_sort(ah_ctx* c, int nkeys, const ah_sort_key* keys, int64_t n, int64_t kk, uint64_t* out) {
  int rc = kk == n ? ah_sort_indices_keys(c, nkeys, keys, n, out) : ah_sort_rows_keys(c, nkeys, keys, nullptr, n, kk, out);
  if (rc != AH_OK) return rc;
  AH_HIP(c, hipStreamSynchronize(c->stream));
  return AH_OK;
}

template <typename T>
int select_radix(ah_ctx* c, int nkeys, const ah_sort_key* keys, int64_t n, int64_t kk, uint64_t* out) {
  const ah_sort_key& k0 = keys[0];
  SelCol<T> col{(const T*)k0.values + k0.off, k0.valid, k0.off, k0.descending, 0ull, 0};
  int rc;
  // ---- classify
  const unsigned sgrid = std::min(ah_stream_grid(c, ah_ceil_div(n, (int64_t)kBlock * kSelUnroll), 8), (unsigned)kSelStatsGrid);
  void* arena;
  {
    TempCarver tc;
    tc.take((size_t)kSelStatsGrid * 8 * 8);
    tc.take((size_t)kSelLevels * kSelBins * 4 + sizeof(SelState));
    if ((rc = ah_temp_reserve(c, tc.used, &arena)) != AH_OK) return rc;
  }
  TempCarver ta;
  ta.base = (uint8_t*)arena;
  unsigned long long* parts_dev = (unsigned long long*)ta.take((size_t)kSelStatsGrid * 8 * 8);
  unsigned* ghist = (unsigned*)ta.take((size_t)kSelLevels * kSelBins * 4 + sizeof(SelState));
  SelState* st_dev = (SelState*)(ghist + kSelLevels * kSelBins);
  sel_classify_kernel<T><<<sgrid, kBlock, 0, c->stream>>>(col, n, parts_dev);
  AH_LAUNCH_CHECK(c);
  std::vector<unsigned long long> parts((size_t)sgrid * 8);
  AH_HIP(c, hipMemcpyAsync(parts.data(), parts_dev, parts.size() * 8, hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipStreamSynchronize(c->stream));
  unsigned long long kmin = ~0ull, kmax = 0, nans = 0, nulls = 0;
  for (unsigned g = 0; g < sgrid; g++) {
    kmin = std::min(kmin, parts[g * 8]); kmax = std::max(kmax, parts[g * 8 + 1]);
    nans += parts[g * 8 + 2]; nulls += parts[g * 8 + 3];
  }
  if ((int64_t)(nans + nulls) > n) return ah_fail(c, AH_EHIP, "select_k: inconsistent category counts");
  const int64_t n_rest = n - (int64_t)nans - (int64_t)nulls;
  // how much of each group the answer holds: [rest, NaNs, nulls] or [nulls, NaNs, rest]
  int64_t k_rest, k_nan, k_null;
  if (k0.nulls_at_start) {
    k_null = std::min(kk, (int64_t)nulls);
    k_nan = std::min(kk - k_null, (int64_t)nans);
    k_rest = kk - k_null - k_nan;
  } else {
    k_rest = std::min(kk, n_rest);
    k_nan = std::min(kk - k_rest, (int64_t)nans);
    k_null = kk - k_rest - k_nan;
  }
  // several keys: the next key orders the NaN and the null group of key 0
  if (nkeys > 1 && (k_nan > 0 || k_null > 0)) return select_by_sort(c, nkeys, keys, n, kk, out);
  // ---- threshold
  SelCut cut{0ull, 0, kModeThreshold};
  unsigned below = 0, take_eq = 0;
  if (k_rest == 0) {
    cut.mode = kModeNoRest;
  } else if (kmax == kmin || k_rest == n_rest) {
    // a constant column: every rest row ties; or every rest row belongs — the first take_eq in row order either way
    cut.mode = kModeAllRest;
    take_eq = (unsigned)(nkeys > 1 ? n_rest : k_rest);
    if (kmax != kmin) { col.kmin = kmin; col.lz = __builtin_clzll(kmax - kmin); }
  } else {
    col.kmin = kmin;
    col.lz = __builtin_clzll(kmax - kmin);
    int nlevels = 1;
    while (nlevels < kSelLevels && sel_level_shift(nlevels - 1) > col.lz) nlevels++;   // bits below lz are zero in every nk
    AH_HIP(c, hipMemsetAsync(ghist, 0, (size_t)kSelLevels * kSelBins * 4 + sizeof(SelState), c->stream));
    const unsigned hgrid = ah_stream_grid(c, ah_ceil_div(n, (int64_t)kBlock * kSelUnroll), 4);
    for (int l = 0; l < nlevels; l++) {
      sel_hist_kernel<T><<<hgrid, kBlock, 0, c->stream>>>(col, n, l, st_dev, ghist + l * kSelBins);
      AH_LAUNCH_CHECK(c);
      sel_pick_kernel<<<1, kBlock, 0, c->stream>>>(ghist + l * kSelBins, st_dev, l, (unsigned)k_rest, l == nlevels - 1, nkeys > 1);
      AH_LAUNCH_CHECK(c);
    }
    AH_HIP(c, hipMemcpyAsync(c->pinned, st_dev, sizeof(SelState), hipMemcpyDeviceToHost, c->stream));
    AH_HIP(c, hipStreamSynchronize(c->stream));
    SelState st;
    memcpy(&st, (const void*)c->pinned, sizeof(st));
    // the buffers below are sized from these numbers: refuse anything the levels cannot have produced
    if (!st.done || (int64_t)st.below >= k_rest || (int64_t)st.below + st.take_eq < k_rest || (int64_t)st.below + st.take_eq > n_rest ||
        st.shift > 53 || (nkeys == 1 && (int64_t)st.below + st.take_eq > k_rest + (int64_t)kSelSmallBin))
      return ah_fail(c, AH_EHIP, "select_k: the threshold levels did not converge");
    cut.prefix = st.prefix;
    cut.shift = (int)st.shift;
    below = st.below;
    take_eq = st.take_eq;
  }
  const int64_t m = (int64_t)below + take_eq;
  if (nkeys > 1 && m > n / kSelCandidateShare) return select_by_sort(c, nkeys, keys, n, kk, out);
  // ---- collect
  const int64_t ntiles = ah_ceil_div(n, (int64_t)kSelTile);
  const int64_t sort_blocks = ah_ceil_div(std::max<int64_t>(m, 1), (int64_t)kTile);
  const bool tied = kmax == kmin;   // a constant column: the pairs are in row order already
  const bool lsd = nkeys == 1 && m > kSelRankSort && !tied;
  unsigned *hist4, *offs4, *pr = nullptr, *ralt = nullptr, *shist = nullptr, *soffs = nullptr;
  unsigned long long *pk = nullptr, *kalt = nullptr;
  auto carve = [&](TempCarver& t) {
    t.take(hist4, (size_t)4 * ntiles);
    t.take(offs4, (size_t)4 * ntiles);
    if (nkeys == 1) {
      t.take(pk, (size_t)m);
      t.take(pr, (size_t)m);
      if (lsd) {
        t.take(kalt, (size_t)m);
        t.take(ralt, (size_t)m);
        t.take(shist, (size_t)kRadix * sort_blocks);
        t.take(soffs, (size_t)kRadix * sort_blocks);
      }
    }
  };
  TempCarver measure;
  carve(measure);
  if ((rc = ah_temp_reserve(c, measure.used, &arena)) != AH_OK) return rc;
  TempCarver tb;
  tb.base = (uint8_t*)arena;
  carve(tb);
  if (nkeys > 1) {   // these outlive the sort of the candidates, which takes the temp arena
    void* pack;
    TempCarver pm;
    pm.take(pk, (size_t)m); pm.take(pr, (size_t)m);
    if ((rc = ah_pack_reserve(c, pm.used, &pack)) != AH_OK) return rc;
    TempCarver pc;
    pc.base = (uint8_t*)pack;
    pc.take(pk, (size_t)m); pc.take(pr, (size_t)m);
  }
  const int64_t pos_rest = k0.nulls_at_start ? k_null + k_nan : 0;
  const int64_t pos_nan = k0.nulls_at_start ? k_null : k_rest;
  const int64_t pos_null = k0.nulls_at_start ? 0 : k_rest + k_nan;
  SelOut so{pk, pr, out + pos_nan, out + pos_null, below, take_eq, (unsigned)k_nan, (unsigned)k_null};
  sel_count_kernel<T><<<(unsigned)ntiles, kBlock, 0, c->stream>>>(col, n, ntiles, cut, hist4);
  AH_LAUNCH_CHECK(c);
  if ((rc = ah_cumulative_sum(c, AH_UINT32, hist4, nullptr, 0, 4 * ntiles, nullptr, 0, 0, offs4, nullptr, nullptr)) != AH_OK) return rc;
  sel_fill_kernel<T><<<(unsigned)ntiles, kBlock, 0, c->stream>>>(col, n, ntiles, cut, hist4, offs4, so);
  AH_LAUNCH_CHECK(c);
  // ---- order
  if (k_rest > 0 && nkeys > 1) {
    if ((rc = ah_sort_rows_keys(c, nkeys, keys, pr, m, k_rest, out + pos_rest)) != AH_OK) return rc;
  } else if (k_rest > 0 && tied) {
    sel_emit_kernel<<<ah_stream_grid(c, ah_ceil_div(k_rest, kBlock), 8), kBlock, 0, c->stream>>>(pr, k_rest, out + pos_rest);
    AH_LAUNCH_CHECK(c);
  } else if (k_rest > 0 && !lsd) {
    sel_bitonic_kernel<<<1, kBlock, 0, c->stream>>>(pk, pr, (int)m, (unsigned)k_rest, out + pos_rest);
    AH_LAUNCH_CHECK(c);
  } else if (k_rest > 0) {
    unsigned long long* kcur = pk;
    unsigned* rcur = pr;
    // every nk is a multiple of 2^lz: the bytes below lz / 8 are zero
    for (int by = col.lz / 8; by < 8; by++) {
      Pairs src{kcur, rcur, 8 * by};
      if ((rc = radix_pass(c, src, m, shist, soffs, kalt, ralt)) != AH_OK) return rc;
      std::swap(kcur, kalt);
      std::swap(rcur, ralt);
    }
    sel_emit_kernel<<<ah_stream_grid(c, ah_ceil_div(k_rest, kBlock), 8), kBlock, 0, c->stream>>>(rcur, k_rest, out + pos_rest);
    AH_LAUNCH_CHECK(c);
  }
  AH_HIP(c, hipStreamSynchronize(c->stream));
  return AH_OK;
}

// AH_SELECT_AUTO: the radix route where the measurement (2^24 and 2^27 rows, k = 10 … n / 16 and n / 2) has it
// ahead of the sort on every column: up to k = n / 16.  At k = n / 2 it is behind on random keys (its ordering step is then an
// LSD sort of half the column), so above n / 16, and below 2^16 rows where nothing was measured, the sort route.
constexpr int kSelAutoShare = 16;
bool auto_takes_radix(int64_t n, int64_t kk) {
  return n >= ((int64_t)1 << 16) && kk <= n / kSelAutoShare;
}

}  // namespace

AH_EXPORT int ah_select_k(ah_ctx* c, int nkeys, const ah_sort_key* keys, int64_t n, int64_t k, int route, uint64_t* out_indices) {
  AH_ENTER(c);
  if (nkeys < 1) return ah_fail(c, AH_EINVALID, "must provide at least one sort key");  // compute/vector_sort.go:119-121
  if (!keys) return ah_fail(c, AH_EINVALID, "select_k: null buffer");
  if (n < 0) return ah_fail(c, AH_EINVALID, "select_k: negative length");
  if (k < 0) return ah_fail(c, AH_EINVALID, "select_k: k must be non-negative, got %lld", (long long)k);
  if (route != AH_SELECT_AUTO && route != AH_SELECT_RADIX && route != AH_SELECT_SORT) return ah_fail(c, AH_EINVALID, "select_k: unknown route %d", route);
  for (int i = 0; i < nkeys; i++)
    if (keys[i].off < 0) return ah_fail(c, AH_EINVALID, "select_k: negative offset");
  const bool numeric = ah_type_width(keys[0].type) != 0;
  if (route == AH_SELECT_RADIX && !numeric)
    return ah_fail(c, AH_ENOTIMPL, "select_k: the radix route takes a numeric first key, not type %d", keys[0].type);
  if (n == 0 || k == 0) return AH_OK;
  if (!out_indices) return ah_fail(c, AH_EINVALID, "select_k: null buffer");
  if (n >= ((int64_t)1 << 32)) return ah_fail(c, AH_ENOTIMPL, "select_k: more than 2^32 - 1 rows in one batch");
  const int64_t kk = std::min(k, n);
  if (route == AH_SELECT_SORT || !numeric || (route == AH_SELECT_AUTO && !auto_takes_radix(n, kk)))
    return select_by_sort(c, nkeys, keys, n, kk, out_indices);
  if (!keys[0].values) return ah_fail(c, AH_EINVALID, "select_k: null buffer");
  if ((uintptr_t)keys[0].values & (uintptr_t)(ah_type_width(keys[0].type) - 1)) return ah_fail(c, AH_EINVALID, "select_k: buffer not element-aligned");
  int rc = AH_ENOTIMPL;
  with_numeric_type(keys[0].type, [&](auto t) { rc = select_radix<typename decltype(t)::type>(c, nkeys, keys, n, kk, out_indices); });
  return rc;
}
