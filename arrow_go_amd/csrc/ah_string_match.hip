// ah_string_match.hip (include/arrowhip_strings.h) — what is inside a string: match_substring, starts_with, ends_with, find_substring, match_like, binary_length,
// utf8_length over String / Binary / LargeString / LargeBinary columns (no reference analogue; Arrow C++'s semantics).
//
// The searches work over the value BYTES of the column, which are contiguous across rows, not over its rows.  The data buffer of the
// call, [offsets[0], offsets[n]), is cut into tiles of T bytes (context option string_tile_bytes, default kDefaultTile); the tile
// count is computed on the device — the host never learns the byte count, no call synchronises — and every workgroup takes a
// contiguous run of tiles.  Per tile:
//   1. stage: the tile's bytes plus the m − 1 behind it (m = pattern length) go into LDS, 16 bytes per lane, coalesced;
//   2. test:  every byte position of the tile is tested in parallel — a thread takes 32 consecutive positions, reads five aligned
//             8-byte words and funnel-shifts the 8-byte window of each position against the pattern's first word (longer patterns are
//             verified word by word where the first word ties) — into one bit per position, a 32-bit word per thread, in LDS
//             (utf8_length: the bit says "not a 10xxxxxx continuation byte");
//   3. rows:  the rows that start in the tile — and the one that reaches in from the tile before — are walked a row per lane over
//             that bit array: first set bit of the row's position range (find), its population count (utf8_length).  A range above
//             kLaneSpan positions is handed to the whole wave, 2048 positions per step, one pending row after another, so a row that
//             fills the tile does not serialise its neighbours.
// A row whose positions all lie in one tile is written by that tile with a plain store.  A row that reaches over a tile border gets
// its result combined from its tiles with atomicMin (find) / atomicAdd (length) on its own output element, which a memset ahead of
// the kernel set to the identity (−1 / 0); at most two rows per tile take that road.  find and the lengths write the caller's output
// directly; the Boolean predicates go through a 4-byte row array in the scratch arena and one packing pass (a ballot per 64 rows,
// put_word: every output word has one owner).
//
// starts_with / ends_with / equals / binary_length touch the offsets and at most m bytes per row: a row per lane, 64 bytes by the
// lane, longer patterns by the whole wave (wave_compare of ah_bytes.h); the pattern sits in LDS.
//
// LIKE: the host compiles the pattern into segments (include/arrowhip.h); programs one simple predicate answers are sent there on the
// host.  Every other program runs in like_kernel: the same tiles, staged with an overlap of T / 4 bytes, the rows that start in a tile
// matched from LDS segment by segment — leftmost-greedy, a row per lane up to kLaneLike bytes, longer rows by the whole wave, 64
// candidate positions of a segment per step.  The one row per tile that ends behind the staged bytes is matched by the wave from
// global memory.  Code-point stepping for `_` on UTF-8 columns is part of the segment walk (seg_fwd / seg_rev).
#include "ah_bytes.h"
#include "ah_strings.h"
#include "../../include/arrowhip_strings.h"

namespace {

constexpr int kLaneSpan = 512;       // positions (16 words of the bit array) a lane scans alone
constexpr int kLaneLike = 256;       // bytes of a row a lane matches alone (LIKE)
constexpr int kLaneCmp = 64;         // bytes of the pattern a lane compares alone (starts_with / ends_with / equals)
constexpr int kMaxLikeElems = 2048, kMaxLikeSegs = 512;
constexpr int kMaxProgram = 3 + 2 * kMaxLikeSegs + 2 * kMaxLikeElems;

enum { kFind = 0, kCount = 1 };

template <int OW>
__device__ __forceinline__ int64_t off_at(const void* offsets, int64_t i) {
  if constexpr (OW == 4) return ((const int32_t*)offsets)[i];
  else return ((const long long*)offsets)[i];
}

__host__ __device__ constexpr int round_up(int x, int to) { return (x + to - 1) / to * to; }

// the LDS image of the searches: [bytes | bit array | pattern words]
__host__ __device__ inline int hit_words(int T) { return (T + 31) >> 5; }
__host__ __device__ inline int stage_bytes(int T, int m) { return round_up(hit_words(T) * 32 + m + 16, 16); }
__host__ __device__ inline int pattern_words(int m) { return (m + 7) / 8 + 1; }

// the run of tiles of this workgroup and its first row: the first row that starts at or behind the run's first byte
template <int OW>
__device__ __forceinline__ bool column_run(const void* offsets, int64_t n, int T, int64_t* base, int64_t* end, int64_t* ntiles, int64_t* t0, int64_t* t1,
                                           long long* s_cur) {
  const int64_t b = *base = off_at<OW>(offsets, 0);
  *end = off_at<OW>(offsets, n);
  const int64_t total = *end - b;
  *ntiles = total > 0 ? (total + T - 1) / T : 1;   // (a column without bytes still has rows to answer: one empty tile)
  if (!tile_run(*ntiles, T, n, [&](int64_t i, int64_t x) { return off_at<OW>(offsets, i) < b + x; }, t0, t1, s_cur)) return false;   // (offsets[n] = end is not in front of x)
  __syncthreads();
  return true;
}

// bytes [tb, tb + avail) of the data buffer into s_data[0 …], zeros behind them up to `bytes` (a multiple of 16)
__device__ __forceinline__ void stage_tile(const uint8_t* __restrict__ data, int64_t tb, int64_t avail, uint8_t* s_data, int bytes) {
  for (int c = threadIdx.x * 16; c < bytes; c += kBlock * 16) {
    if (c + 16 <= avail) {
      const ah_vec16<uint8_t> v = ah_ld16<uint8_t>(data + tb + c);
      uint4 q;
      __builtin_memcpy(&q, &v, 16);
      *(uint4*)(s_data + c) = q;
    } else {
      for (int k = 0; k < 16; k++) s_data[c + k] = c + k < avail ? data[tb + c + k] : (uint8_t)0;
    }
  }
}

// the 8 bytes at s_data + pos (any pos) from two aligned words
__device__ __forceinline__ unsigned long long window8(const uint8_t* s_data, int pos) {
  const unsigned long long* w = (const unsigned long long*)(s_data + (pos & ~7));
  const int s = (pos & 7) * 8;
  return s ? (w[0] >> s) | (w[1] << (64 - s)) : w[0];
}

// one bit per position 32 w … 32 w + 31 of the staged tile: the pattern's m bytes stand there
__device__ __forceinline__ unsigned hit_word_find(const uint8_t* s_data, const unsigned long long* s_pat, int m, int w) {
  const unsigned long long* W = (const unsigned long long*)(s_data + w * 32);
  unsigned long long x[5];
#pragma unroll
  for (int k = 0; k < 5; k++) x[k] = W[k];
  const unsigned long long p0 = s_pat[0];
  const unsigned long long mask0 = m >= 8 ? ~0ull : ((1ull << (8 * m)) - 1);
  unsigned bits = 0;
#pragma unroll
  for (int j = 0; j < 32; j++) {
    const int k = j >> 3, s = (j & 7) * 8;
    const unsigned long long win = s ? (x[k] >> s) | (x[k + 1] << (64 - s)) : x[k];
    if (((win ^ p0) & mask0) == 0) {
      bool ok = true;
      for (int q = 8; q < m && ok; q += 8) {
        const unsigned long long mk = m - q >= 8 ? ~0ull : ((1ull << (8 * (m - q))) - 1);
        ok = ((window8(s_data, w * 32 + j + q) ^ s_pat[q >> 3]) & mk) == 0;
      }
      if (ok) bits |= 1u << j;
    }
  }
  return bits;
}

// … the byte there is not a UTF-8 continuation byte (10xxxxxx)
__device__ __forceinline__ unsigned hit_word_lead(const uint8_t* s_data, int w) {
  const unsigned long long* W = (const unsigned long long*)(s_data + w * 32);
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const unsigned long long x = W[k];
    const unsigned long long cont = (x >> 7) & ~(x >> 6) & 0x0101010101010101ull;   // bit 8 b: byte b is 10xxxxxx
    const unsigned long long lead = cont ^ 0x0101010101010101ull;
    bits |= (unsigned)((lead * 0x0102040810204080ull) >> 56) << (8 * k);            // the eight flags gathered into one byte
  }
  return bits;
}

// word k of the bit array cut to the positions [a, b)
__device__ __forceinline__ unsigned range_word(const unsigned* h, int k, int a, int b) {
  unsigned w = h[k];
  if (k == (a >> 5)) w &= ~0u << (a & 31);
  if (k == ((b - 1) >> 5) && (b & 31)) w &= ~0u >> (32 - (b & 31));
  return w;
}

// positions [a, b) of the bit array, a < b: the first set one or −1 (kFind), how many are set (kCount) — by one lane
template <int MODE>
__device__ __forceinline__ int scan_lane(const unsigned* h, int a, int b) {
  const int k1 = (b - 1) >> 5;
  int r = MODE == kFind ? -1 : 0;
  for (int k = a >> 5; k <= k1; k++) {
    const unsigned w = range_word(h, k, a, b);
    if (MODE == kFind) {
      if (w) return k * 32 + __ffs((int)w) - 1;
    } else {
      r += __popc(w);
    }
  }
  return r;
}

// … by the whole wave for the lanes in `need` (wave-uniform; all 64 lanes call), 64 words = 2048 positions per step
template <int MODE>
__device__ __forceinline__ void scan_wave(unsigned long long need, const unsigned* h, int a, int b, int* res) {
  const int lane = ah_lane();
  for_pending_lanes(need, [&](int l) {
    const int ra = __shfl(a, l), rb = __shfl(b, l);
    const int k1 = (rb - 1) >> 5;
    int r = MODE == kFind ? -1 : 0;
    for (int kb = ra >> 5; kb <= k1; kb += 64) {
      const int k = kb + lane;
      const unsigned w = k <= k1 ? range_word(h, k, ra, rb) : 0u;
      if (MODE == kFind) {
        const unsigned long long any = __ballot(w != 0);
        if (any) {
          r = __shfl(k * 32 + __ffs((int)w) - 1, __ffsll((long long)any) - 1);
          break;
        }
      } else {
        r += __popc(w);
      }
    }
    if (MODE == kCount) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) r += __shfl_xor(r, o);
    }
    if (lane == l) *res = r;
  });
}

// The search over the tiles.  MODE kFind: out[i] = the byte index of the pattern's first occurrence in row i, all ones for none;
// kCount: the row's bytes that are not continuation bytes (m = 1).  `out` holds the identity (all ones / 0) when the kernel starts.
template <int OW, int MODE, typename OutT>
__global__ __launch_bounds__(kBlock) void search_kernel(const void* __restrict__ offsets, const uint8_t* __restrict__ data, int64_t n,
                                                        const unsigned long long* __restrict__ pat, int m, int T, OutT* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  __shared__ long long s_cur;
  const int nwords = hit_words(T), sbytes = stage_bytes(T, m);
  uint8_t* s_data = lds;
  unsigned* s_hit = (unsigned*)(lds + sbytes);
  unsigned long long* s_pat = (unsigned long long*)(lds + sbytes + round_up(nwords * 4, 8));
  int64_t base, end, ntiles, t0, t1;
  if (!column_run<OW>(offsets, n, T, &base, &end, &ntiles, &t0, &t1, &s_cur)) return;
  if (MODE == kFind)
    for (int j = threadIdx.x; j < pattern_words(m); j += kBlock) s_pat[j] = pat[j];
  int64_t cur = s_cur;
  for (int64_t t = t0; t < t1; t++) {
    const int64_t tb = base + t * T, te = tb + T;
    const bool last = t == ntiles - 1;
    int64_t avail = end - tb;
    if (avail > (int64_t)T + m - 1) avail = (int64_t)T + m - 1;
    stage_tile(data, tb, avail, s_data, sbytes);
    __syncthreads();
    for (int w = threadIdx.x; w < nwords; w += kBlock) s_hit[w] = MODE == kFind ? hit_word_find(s_data, s_pat, m, w) : hit_word_lead(s_data, w);
    __syncthreads();
    // the rows: the one that reaches in from before the tile (row cur − 1, when it exists), then those that start in it
    const int64_t i0 = cur > 0 ? cur - 1 : 0;
    int64_t seen = 0;
    for (int64_t it = i0;; it += kBlock) {
      const int64_t i = it + threadIdx.x;
      bool in = false, pend = false;
      int64_t rs = 0, re = 0;
      int a = 0, b = 0, r = MODE == kFind ? -1 : 0;
      if (i < n) {
        rs = off_at<OW>(offsets, i);
        in = last || rs < te;
      }
      if (in) {
        re = off_at<OW>(offsets, i + 1);
        const int64_t lo = rs > tb ? rs : tb, hi = re - m + 1 < te ? re - m + 1 : te;   // the row's pattern positions inside this tile
        if (hi > lo) {
          a = (int)(lo - tb);
          b = (int)(hi - tb);
          if (b - a <= kLaneSpan) r = scan_lane<MODE>(s_hit, a, b);
          else pend = true;
        }
      }
      scan_wave<MODE>(__ballot(pend), s_hit, a, b, &r);
      if (in) {
        const bool whole = rs >= tb && re - m + 1 <= te;   // every position of the row lies in this tile: this thread owns out[i]
        if (MODE == kFind) {
          const OutT v = r < 0 ? (OutT)~(OutT)0 : (OutT)(tb + r - rs);
          if (whole) out[i] = v;
          else if (r >= 0) atomicMin(&out[i], v);
        } else {
          if (whole) out[i] = (OutT)r;
          else if (r > 0) atomicAdd(&out[i], (OutT)r);
        }
      }
      const int cnt = __syncthreads_count(in);
      seen += cnt;
      if (cnt < kBlock) break;
    }
    cur = i0 + seen;
  }
}

// the Boolean of a search: bit i = part[i] is not `none`
template <typename PartT>
__global__ __launch_bounds__(kBlock) void pack_kernel(const PartT* __restrict__ part, PartT none, int64_t n, uint8_t* __restrict__ out, int64_t out_off,
                                                      int aligned) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const int cnt = left >= 64 ? 64 : (int)left;
    const unsigned long long word = __ballot(lane < cnt && part[row] != none);
    if (lane == 0) put_word(out, out_off, aligned, ch, word, cnt);
  }
}

// ---- starts_with / ends_with / equals: the offsets and at most m bytes per row ----------------------------------------------------------
template <int OW>
__global__ __launch_bounds__(kBlock) void edge_kernel(ByteRows rows, int op, int64_t n, const unsigned long long* __restrict__ pat, int m,
                                                      uint8_t* __restrict__ out, int64_t out_off, int aligned) {
  __shared__ unsigned long long s_pat[AH_STR_MAX_PATTERN / 8 + 1];
  for (int j = threadIdx.x; j < pattern_words(m); j += kBlock) s_pat[j] = pat[j];
  __syncthreads();
  const uint8_t* q = (const uint8_t*)s_pat;
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const int cnt = left >= 64 ? 64 : (int)left;
    const uint8_t* p = nullptr;
    int64_t len = 0;
    bool hit = false, pend = false;
    if (lane < cnt) {
      row_at<OW>(rows, row, &p, &len);
      if (op == AH_STR_EQUALS ? len == m : len >= m) {
        if (op == AH_STR_ENDS_WITH) p += len - m;
        const int first = m < kLaneCmp ? m : kLaneCmp;
        hit = true;
        for (int j = 0; j < first && hit; j += 8) hit = word_at(p, j, m) == s_pat[j >> 3];   // (the pattern is zero-padded, as word_at pads)
        pend = hit && m > kLaneCmp;
      }
    }
    wave_compare<false>(__ballot(pend), p, q, m, kLaneCmp, [&](int r) { hit = r == 0; });
    const unsigned long long word = __ballot(hit);
    if (lane == 0) put_word(out, out_off, aligned, ch, word, cnt);
  }
}

// binary_length: the difference of two offsets, or the slot width
template <int OW, typename OutT>
__global__ __launch_bounds__(kBlock) void length_kernel(ByteRows rows, int64_t n, OutT* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const uint8_t* p;
    int64_t len;
    row_at<OW>(rows, i, &p, &len);
    out[i] = (OutT)len;
  }
}

// ---- LIKE ------------------------------------------------------------------------------------------------------------------------------
// One segment of the program: a 2-byte element count, then {kind, byte} pairs (kind 0: the literal byte, 1: one character).
// `_` on a UTF-8 column is one byte that is not 10xxxxxx and ALL the continuation bytes behind it, read forwards or backwards.

// the segment matched at position x of the row's first `len` bytes → the position behind it, or −1
__device__ __forceinline__ long long seg_fwd(const uint8_t* seg, const uint8_t* p, long long x, long long len, int utf8) {
  const int ne = seg[0] | (seg[1] << 8);
  for (int e = 0; e < ne; e++) {
    if (x >= len) return -1;
    if (seg[2 + 2 * e] == 0) {
      if (p[x] != seg[3 + 2 * e]) return -1;
      x++;
    } else if (!utf8) {
      x++;
    } else {
      if (is_cont(p[x])) return -1;
      x++;
      while (x < len && is_cont(p[x])) x++;
    }
  }
  return x;
}
// the segment matched so that it ends at position x (x ≤ len, the row's length) → where it starts, or −1
__device__ __forceinline__ long long seg_rev(const uint8_t* seg, const uint8_t* p, long long x, long long len, int utf8) {
  const int ne = seg[0] | (seg[1] << 8);
  for (int e = ne - 1; e >= 0; e--) {
    if (x <= 0) return -1;
    if (seg[2 + 2 * e] == 0) {
      if (p[x - 1] != seg[3 + 2 * e]) return -1;
      x--;
    } else if (!utf8) {
      x--;
    } else {
      if (x < len && is_cont(p[x])) return -1;   // the character would go on behind x
      x--;
      while (x > 0 && is_cont(p[x])) x--;
      if (is_cont(p[x])) return -1;
    }
  }
  return x;
}

// The row (p, len) against the program, leftmost-greedy.  WAVE: all 64 lanes hold the same row and test 64 candidate positions of a
// middle segment per step; else one lane walks alone.
template <bool WAVE>
__device__ __forceinline__ bool like_row(const uint8_t* prog, const unsigned short* seg_pos, const uint8_t* p, long long len, int utf8) {
  const int flags = prog[0], nseg = prog[1] | (prog[2] << 8);
  if (nseg == 0) return true;
  if (nseg == 1 && (flags & AH_LIKE_ANCHOR_START) && (flags & AH_LIKE_ANCHOR_END)) return seg_fwd(prog + seg_pos[0], p, 0, len, utf8) == len;
  long long pos = 0, lim = len;
  int s0 = 0, s1 = nseg;
  if (flags & AH_LIKE_ANCHOR_START) {
    pos = seg_fwd(prog + seg_pos[0], p, 0, len, utf8);
    if (pos < 0) return false;
    s0 = 1;
  }
  if (flags & AH_LIKE_ANCHOR_END) {
    lim = seg_rev(prog + seg_pos[nseg - 1], p, len, len, utf8);
    if (lim < pos) return false;   // (−1 included)
    s1 = nseg - 1;
  }
  for (int s = s0; s < s1; s++) {
    const uint8_t* seg = prog + seg_pos[s];
    long long found = -1;
    if (WAVE) {
      const int lane = ah_lane();
      for (long long x0 = pos; x0 <= lim; x0 += 64) {
        const long long x = x0 + lane;
        const long long e = x <= lim ? seg_fwd(seg, p, x, lim, utf8) : -1;
        const unsigned long long any = __ballot(e >= 0);
        if (any) {
          found = __shfl(e, __ffsll((long long)any) - 1);
          break;
        }
      }
    } else {
      for (long long x = pos; x <= lim && found < 0; x++) found = seg_fwd(seg, p, x, lim, utf8);
    }
    if (found < 0) return false;
    pos = found;
  }
  return true;
}

template <int OW>
__global__ __launch_bounds__(kBlock) void like_kernel(const void* __restrict__ offsets, const uint8_t* __restrict__ data, int64_t n,
                                                      const uint8_t* __restrict__ program, int program_len, int utf8, int T, int overlap,
                                                      uint8_t* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  __shared__ long long s_cur;
  __shared__ uint8_t s_prog[round_up(kMaxProgram, 8)];
  __shared__ unsigned short s_seg[kMaxLikeSegs];
  const int sbytes = round_up(T + overlap, 16);
  uint8_t* s_data = lds;
  int64_t base, end, ntiles, t0, t1;
  if (!column_run<OW>(offsets, n, T, &base, &end, &ntiles, &t0, &t1, &s_cur)) return;
  for (int j = threadIdx.x; j < program_len; j += kBlock) s_prog[j] = program[j];
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nseg = s_prog[1] | (s_prog[2] << 8);
    int at = 3;
    for (int s = 0; s < nseg; s++) {
      s_seg[s] = (unsigned short)at;
      at += 2 + 2 * (s_prog[at] | (s_prog[at + 1] << 8));
    }
  }
  int64_t cur = s_cur;
  for (int64_t t = t0; t < t1; t++) {
    const int64_t tb = base + t * T, te = tb + T;
    const bool last = t == ntiles - 1;
    int64_t avail = end - tb;
    if (avail > (int64_t)T + overlap) avail = (int64_t)T + overlap;
    __syncthreads();   // the rows of the tile before are through with s_data (and s_seg is written)
    stage_tile(data, tb, avail, s_data, sbytes);
    __syncthreads();
    int64_t seen = 0;
    for (int64_t it = cur;; it += kBlock) {   // the rows that start in this tile
      const int64_t i = it + threadIdx.x;
      bool in = false, pend = false, hit = false;
      const uint8_t* p = nullptr;
      long long len = 0;
      if (i < n) {
        const int64_t rs = off_at<OW>(offsets, i);
        in = last || rs < te;
        if (in) {
          const int64_t re = off_at<OW>(offsets, i + 1);
          len = re - rs;
          p = re <= tb + avail ? s_data + (rs - tb) : data + rs;   // the row's bytes are staged, or it ends behind them
          if (len <= kLaneLike) hit = like_row<false>(s_prog, s_seg, p, len, utf8);
          else pend = true;
        }
      }
      for_pending_lanes(__ballot(pend), [&](int l) {   // the long rows: the whole wave, one after another
        const uint8_t* wp = (const uint8_t*)(uintptr_t)__shfl((long long)(uintptr_t)p, l);
        const long long wl = __shfl(len, l);
        const bool r = like_row<true>(s_prog, s_seg, wp, wl, utf8);
        if (ah_lane() == l) hit = r;
      });
      if (in) part[i] = hit ? 1 : 0;
      const int cnt = __syncthreads_count(in);
      seen += cnt;
      if (cnt < kBlock) break;
    }
    cur += seen;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
int out_aligned(const uint8_t* out, int64_t out_off) { return (out_off & 63) == 0 && ((uintptr_t)out & 7) == 0; }

int check_pattern(ah_ctx* c, const char* fn, const uint8_t* pattern, int64_t m) {
  if (m < 0 || m > AH_STR_MAX_PATTERN) return ah_fail(c, AH_EINVALID, "%s: pattern length %lld outside 0 … %d", fn, (long long)m, AH_STR_MAX_PATTERN);
  if (m > 0 && !pattern) return ah_fail(c, AH_EINVALID, "%s: null pattern", fn);
  return AH_OK;
}
int check_out_width(ah_ctx* c, const char* fn, const ah_cmp_operand* o, int out_width, const void* out, int64_t n) {
  if (out_width != 4 && out_width != 8) return ah_fail(c, AH_EINVALID, "%s: output width must be 4 or 8 (got %d)", fn, out_width);
  if (o->offset_width == 8 && out_width != 8) return ah_fail(c, AH_EINVALID, "%s: a column with 8-byte offsets needs an 8-byte output", fn);
  if (n > 0 && (!out || ((uintptr_t)out & (uintptr_t)(out_width - 1)))) return ah_fail(c, AH_EINVALID, "%s: null or misaligned output", fn);
  return AH_OK;
}
int check_bits(ah_ctx* c, const char* fn, const uint8_t* out_bits, int64_t out_bit_offset, int64_t n) {
  if (out_bit_offset < 0) return ah_fail(c, AH_EINVALID, "%s: negative output bit offset", fn);
  if (n > 0 && !out_bits) return ah_fail(c, AH_EINVALID, "%s: null output bitmap", fn);
  return AH_OK;
}

// the pattern as zero-padded 8-byte words on the device, in front of `extra` more bytes of the scratch arena
int upload_pattern(ah_ctx* c, const uint8_t* pattern, int m, size_t extra, unsigned long long** pat, uint8_t** rest) {
  const size_t pbytes = (size_t)pattern_words(m) * 8;
  void* tmp = nullptr;
  if (int rc = ah_scratch_reserve(c, ah_pad(pbytes) + extra, &tmp)) return rc;
  *pat = (unsigned long long*)tmp;
  *rest = (uint8_t*)tmp + ah_pad(pbytes);
  AH_HIP(c, hipMemsetAsync(tmp, 0, pbytes, c->stream));
  if (m > 0) AH_HIP(c, hipMemcpyAsync(tmp, pattern, (size_t)m, hipMemcpyHostToDevice, c->stream));
  return AH_OK;
}

template <int MODE, typename OutT>
int launch_search(ah_ctx* c, const ah_cmp_operand* o, int64_t n, const unsigned long long* pat, int m, OutT* out) {
  const int T = tile_bytes(c);
  const size_t lds = (size_t)stage_bytes(T, m) + round_up(hit_words(T) * 4, 8) + (size_t)pattern_words(m) * 8;
  AH_HIP(c, hipMemsetAsync(out, MODE == kFind ? 0xFF : 0, (size_t)n * sizeof(OutT), c->stream));
  const ByteRows rows = byte_rows(o->offset_width, o->offsets, o->data, 0, o->off);
  if (o->offset_width == 4) search_kernel<4, MODE, OutT><<<tile_grid(c), kBlock, lds, c->stream>>>(rows.offsets, rows.data, n, pat, m, T, out);
  else search_kernel<8, MODE, OutT><<<tile_grid(c), kBlock, lds, c->stream>>>(rows.offsets, rows.data, n, pat, m, T, out);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

// the four predicates of ah_string_match, arguments checked
int match_checked(ah_ctx* c, int op, const ah_cmp_operand* o, int64_t n, const uint8_t* pattern, int m, uint8_t* out_bits, int64_t out_bit_offset) {
  if (op != AH_STR_EQUALS && m == 0) return ah_set_bits_to(c, out_bits, out_bit_offset, n, 1);   // the empty pattern is in, before and behind every row
  const int aligned = out_aligned(out_bits, out_bit_offset);
  unsigned long long* pat;
  uint8_t* rest;
  if (int rc = upload_pattern(c, pattern, m, op == AH_STR_SUBSTRING ? (size_t)n * 4 : 0, &pat, &rest)) return rc;
  if (op == AH_STR_SUBSTRING) {
    if (int rc = launch_search<kFind, unsigned>(c, o, n, pat, m, (unsigned*)rest)) return rc;
    pack_kernel<unsigned><<<chunk_grid(c, n), kBlock, 0, c->stream>>>((const unsigned*)rest, ~0u, n, out_bits, out_bit_offset, aligned);
  } else {
    const ByteRows rows = byte_rows(o->offset_width, o->offsets, o->data, 0, o->off);
    if (o->offset_width == 4) edge_kernel<4><<<chunk_grid(c, n), kBlock, 0, c->stream>>>(rows, op, n, pat, m, out_bits, out_bit_offset, aligned);
    else edge_kernel<8><<<chunk_grid(c, n), kBlock, 0, c->stream>>>(rows, op, n, pat, m, out_bits, out_bit_offset, aligned);
  }
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

}  // namespace

AH_EXPORT int ah_string_match(ah_ctx* c, int op, const ah_cmp_operand* operand, int64_t n, const uint8_t* pattern, int64_t pattern_len,
                              uint8_t* out_bits, int64_t out_bit_offset) {
  AH_ENTER(c);
  if (op < AH_STR_SUBSTRING || op > AH_STR_EQUALS) return ah_fail(c, AH_EINVALID, "string_match: bad op %d", op);
  if (int rc = check_column(c, "string_match", operand, n, false)) return rc;
  if (int rc = check_pattern(c, "string_match", pattern, pattern_len)) return rc;
  if (int rc = check_bits(c, "string_match", out_bits, out_bit_offset, n)) return rc;
  if (n == 0) return AH_OK;
  return match_checked(c, op, operand, n, pattern, (int)pattern_len, out_bits, out_bit_offset);
}

AH_EXPORT int ah_string_find(ah_ctx* c, const ah_cmp_operand* operand, int64_t n, const uint8_t* pattern, int64_t pattern_len, int out_width,
                             void* out) {
  AH_ENTER(c);
  if (int rc = check_column(c, "string_find", operand, n, false)) return rc;
  if (int rc = check_pattern(c, "string_find", pattern, pattern_len)) return rc;
  if (int rc = check_out_width(c, "string_find", operand, out_width, out, n)) return rc;
  if (n == 0) return AH_OK;
  const int m = (int)pattern_len;
  if (m == 0) {   // the empty pattern stands at index 0 of every row
    AH_HIP(c, hipMemsetAsync(out, 0, (size_t)n * (size_t)out_width, c->stream));
    return AH_OK;
  }
  unsigned long long* pat;
  uint8_t* rest;
  if (int rc = upload_pattern(c, pattern, m, 0, &pat, &rest)) return rc;
  return out_width == 4 ? launch_search<kFind, unsigned>(c, operand, n, pat, m, (unsigned*)out)
                        : launch_search<kFind, unsigned long long>(c, operand, n, pat, m, (unsigned long long*)out);
}

AH_EXPORT int ah_string_length(ah_ctx* c, const ah_cmp_operand* operand, int64_t n, int utf8, int out_width, void* out) {
  AH_ENTER(c);
  if (int rc = check_column(c, "string_length", operand, n, !utf8)) return rc;
  if (int rc = check_out_width(c, "string_length", operand, out_width, out, n)) return rc;
  if (n == 0) return AH_OK;
  if (utf8)
    return out_width == 4 ? launch_search<kCount, unsigned>(c, operand, n, nullptr, 1, (unsigned*)out)
                          : launch_search<kCount, unsigned long long>(c, operand, n, nullptr, 1, (unsigned long long*)out);
  if (operand->offset_width == 0 && operand->byte_width > 0 && !operand->data) return ah_fail(c, AH_EINVALID, "string_length: null data");
  const ByteRows rows = byte_rows(operand->offset_width, operand->offsets, operand->data, operand->byte_width, operand->off);
  const unsigned grid = ah_stream_grid(c, ah_ceil_div(n, kBlock), 8);
  const int ow = operand->offset_width;
  if (out_width == 4) {
    if (ow == 4) length_kernel<4, int32_t><<<grid, kBlock, 0, c->stream>>>(rows, n, (int32_t*)out);
    else length_kernel<0, int32_t><<<grid, kBlock, 0, c->stream>>>(rows, n, (int32_t*)out);
  } else {
    if (ow == 4) length_kernel<4, long long><<<grid, kBlock, 0, c->stream>>>(rows, n, (long long*)out);
    else if (ow == 8) length_kernel<8, long long><<<grid, kBlock, 0, c->stream>>>(rows, n, (long long*)out);
    else length_kernel<0, long long><<<grid, kBlock, 0, c->stream>>>(rows, n, (long long*)out);
  }
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

AH_EXPORT int ah_string_like(ah_ctx* c, const ah_cmp_operand* operand, int64_t n, int utf8, const uint8_t* program, int64_t program_len,
                             uint8_t* out_bits, int64_t out_bit_offset) {
  AH_ENTER(c);
  if (int rc = check_column(c, "string_like", operand, n, false)) return rc;
  if (int rc = check_bits(c, "string_like", out_bits, out_bit_offset, n)) return rc;
  if (!program || program_len < 3 || program_len > kMaxProgram) return ah_fail(c, AH_EINVALID, "string_like: program of %lld bytes (3 … %d)", (long long)program_len, kMaxProgram);
  // walk the program: every segment inside it, the limits kept; literal-only programs of one segment are a simpler predicate's
  const int flags = program[0], nseg = program[1] | (program[2] << 8);
  if (flags & ~(AH_LIKE_ANCHOR_START | AH_LIKE_ANCHOR_END)) return ah_fail(c, AH_EINVALID, "string_like: unknown program flags %d", flags);
  if (nseg > kMaxLikeSegs) return ah_fail(c, AH_EINVALID, "string_like: %d segments (at most %d)", nseg, kMaxLikeSegs);
  int64_t at = 3, elems = 0;
  bool literal = true;
  for (int s = 0; s < nseg; s++) {
    if (at + 2 > program_len) return ah_fail(c, AH_EINVALID, "string_like: truncated program");
    const int ne = program[at] | (program[at + 1] << 8);
    if (at + 2 + 2 * (int64_t)ne > program_len) return ah_fail(c, AH_EINVALID, "string_like: truncated program");
    if (ne == 0 && nseg > 1) return ah_fail(c, AH_EINVALID, "string_like: empty segment");
    for (int e = 0; e < ne; e++) {
      const int kind = program[at + 2 + 2 * e];
      if (kind > 1) return ah_fail(c, AH_EINVALID, "string_like: unknown element kind %d", kind);
      if (kind == 1) literal = false;
    }
    elems += ne;
    at += 2 + 2 * (int64_t)ne;
  }
  if (at != program_len) return ah_fail(c, AH_EINVALID, "string_like: %lld bytes behind the last segment", (long long)(program_len - at));
  if (elems > kMaxLikeElems) return ah_fail(c, AH_EINVALID, "string_like: pattern of %lld characters (at most %d)", (long long)elems, kMaxLikeElems);
  const bool as = flags & AH_LIKE_ANCHOR_START, ae = flags & AH_LIKE_ANCHOR_END;
  if (nseg == 0 && (as || ae)) return ah_fail(c, AH_EINVALID, "string_like: anchors without a segment");
  if (n == 0) return AH_OK;
  if (nseg == 0) return ah_set_bits_to(c, out_bits, out_bit_offset, n, 1);   // `%`
  if (nseg == 1 && literal) {   // `lit`, `lit%`, `%lit`, `%lit%`
    uint8_t lit[kMaxLikeElems];
    const int m = (int)elems;
    for (int e = 0; e < m; e++) lit[e] = program[3 + 2 + 2 * e + 1];
    const int op = as && ae ? AH_STR_EQUALS : as ? AH_STR_STARTS_WITH : ae ? AH_STR_ENDS_WITH : AH_STR_SUBSTRING;
    return match_checked(c, op, operand, n, lit, m, out_bits, out_bit_offset);
  }
  const int T = tile_bytes(c), overlap = T / 4 < 64 ? 64 : T / 4;
  void* tmp = nullptr;
  if (int rc = ah_scratch_reserve(c, ah_pad((size_t)program_len) + (size_t)n, &tmp)) return rc;
  uint8_t* part = (uint8_t*)tmp + ah_pad((size_t)program_len);
  AH_HIP(c, hipMemcpyAsync(tmp, program, (size_t)program_len, hipMemcpyHostToDevice, c->stream));
  const ByteRows rows = byte_rows(operand->offset_width, operand->offsets, operand->data, 0, operand->off);
  const size_t lds = (size_t)round_up(T + overlap, 16);
  if (operand->offset_width == 4)
    like_kernel<4><<<tile_grid(c), kBlock, lds, c->stream>>>(rows.offsets, rows.data, n, (const uint8_t*)tmp, (int)program_len, utf8 ? 1 : 0, T, overlap, part);
  else
    like_kernel<8><<<tile_grid(c), kBlock, lds, c->stream>>>(rows.offsets, rows.data, n, (const uint8_t*)tmp, (int)program_len, utf8 ? 1 : 0, T, overlap, part);
  pack_kernel<uint8_t><<<chunk_grid(c, n), kBlock, 0, c->stream>>>(part, (uint8_t)0, n, out_bits, out_bit_offset, out_aligned(out_bits, out_bit_offset));
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}
