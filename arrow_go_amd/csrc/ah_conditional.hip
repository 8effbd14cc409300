// ah_conditional.hip — the conditionals: if_else over fixed-width, boolean and var-length columns, and the directed null fills
// (DESIGN.md §3.16).
//
// No reference analogue (arrow-go has no if_else / coalesce / fill_null kernels); the semantics are Arrow C++'s:
//   if_else(cond, l, r)   row i is null where cond[i] is null, otherwise l[i] or r[i] with that side's validity;
//   fill_null_forward / _backward   a null row takes the nearest valid row before / after it and stays null when there is none.
// coalesce and fill_null are folds of if_else on the host (cond_data = the left argument's validity bitmap): no kernel of their own.
// Where Arrow leaves bytes unspecified this library does not: the payload under a null slot of a fixed-width output is zero, a
// null data bit is 0, a null var-length row has length 0.
//
//   ah_if_else                 one streaming pass.  A lane holds 16 bytes of each side (V = 16 / width rows; one row of a 16- or
//                              32-byte slot) per step and kUnroll steps in flight; the bits of a wave's 64·V consecutive rows come
//                              out of the three input bitmaps — at three independent offsets — as wave-uniform 64-bit words
//                              (scalar loads), and the output validity leaves as whole bytes: the 8 / V lanes of a byte fold their
//                              bits with shuffles and ONE of them stores it.  No byte has two writers, so there are no atomics and
//                              the tail is exactly ceil(n / 8) validity bytes and n·width value bytes.  Any other width: a row per
//                              lane over the byte-row layer (ah_bytes.h), as Take does.
//   ah_if_else_boolean         a thread per 64-bit output word: (c & l) | (~c & r) on data and validity.
//   ah_if_else_binary_offsets  lengths of the chosen rows → ah_cumulative_sum → offsets, total to the host (the caller allocates) …
//   ah_if_else_binary_data     … and the bytes: the row copy of the var-length Take (wave_copy_rows, ah_bytes.h).
//   ah_fill_null_indices       per row the number of the row it takes its value from, in the form Take reads as (idx, ivalid);
//   ah_fill_null_directed      the same walk with the gather fused in for 1 / 2 / 4 / 8 / 16 / 32-byte values.
//
// The fills work on the validity bitmap's 64-bit words (word j = rows 64j … 64j + 63 of the call).  Inside a word the source of
// a row is a masked count-leading-zeros (forward) or count-trailing-zeros (backward).  Across words it is the exclusive running
// maximum of one key per word — forward: (last valid row of the word) + 1 scanned from the left, backward: ~(first valid row of
// the word) scanned from the right, 0 for a word without a valid row — so one max-scan serves both directions.  It is done
// reduce-then-scan, as ah_window.hip does and for the reasons recorded in ah_scan.hip:
//   1. carry_reduce_kernel   the key of each workgroup's kCarryRows rows
//   2. carry_prefix_kernel   the exclusive scan of those keys, one workgroup (≤ 2^32 / kCarryRows = 65536 keys)
//   3. fill_kernel           the words of the workgroup's rows scanned in LDS behind that prefix (this pass writes the validity:
//                            a thread owns the eight bytes of its words), then the rows streamed in coalesced order
// No workgroup waits for another one.  A column of one workgroup's rows is launch 3 alone.
#include "ah_bytes.h"
#include "ah_index.h"
#include "ah_varout.h"

namespace {

constexpr int kBlock = 256;
constexpr int kUnroll = 4;           // 16-byte steps a lane of ah_if_else has in flight: a workgroup owns kBlock * kUnroll * V rows
constexpr int kCarryWords = 4;       // validity words per thread in the fills' passes
constexpr int kCarryRows = 65536;    // rows of one workgroup of the fills' passes
static_assert(kCarryRows == kBlock * kCarryWords * 64, "a workgroup of the carry passes owns kBlock * kCarryWords words");
constexpr int kPrefixBlock = 1024;
constexpr int64_t kFillMaxRows = 0xFFFFFFFFll;   // row numbers + 1 travel in 32 bits

typedef unsigned long long u64;

// the condition of a call, and one side as the kernels read it (the array offset applied to the rows, not to the validity)
struct Cond {
  const uint8_t* data;
  const uint8_t* valid;
  int64_t off;
};
struct Side {
  ByteRows rows;          // row 0 of the call first (a broadcast side: its one row)
  int ow;                 // 4 / 8: offsets, 0: fixed slots
  const uint8_t* valid;
  int64_t off;
  int broadcast;
};

// ---- ah_if_else: the vector path ------------------------------------------------------------------------------------------------
// the bits of this lane's V rows out of the wave's 64·V consecutive rows whose first is bit pos0 of `bm`; `left`: rows from that
// first row to the end of the column (both wave-uniform).  Rows past the end read 0, a NULL bitmap reads 1.
// ah_wave_bits64 (ah_common.h) through the constant address space: 64 rows of an INPUT bitmap from the wave-uniform bit position
// `pos`, `left` rows to the column's end.  The kernel writes none of its input bitmaps (buffers do not alias), so the words may
// come through the scalar cache: with the address in scalar registers these are s_load instructions, off the vector memory path
// the streams run on.  Whole aligned 8-byte words that hold at least one of the bits, like ah_load_bits64.
__device__ __forceinline__ u64 wave_bits64_const(const uint8_t* __restrict__ bm, int64_t pos, int64_t left) {
  typedef const __attribute__((address_space(4))) u64 ConstWord;
  const int64_t p = ((int64_t)__builtin_amdgcn_readfirstlane((int)(pos >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)pos);
  const int64_t l = ((int64_t)__builtin_amdgcn_readfirstlane((int)(left >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)left);
  const int nvalid = l >= 64 ? 64 : (int)(l < 0 ? 0 : l);
  if (nvalid <= 0) return 0;
  const u64 mask = nvalid >= 64 ? ~0ull : ((1ull << nvalid) - 1);
  if (bm == nullptr) return mask;
  const uintptr_t addr = (uintptr_t)bm + (uintptr_t)(p >> 3), base = addr & ~(uintptr_t)7;
  const int shift = (int)((addr - base) * 8 + (p & 7));   // 0 … 63
  ConstWord* w = (ConstWord*)base;
  u64 lo = w[0] >> shift;
  if (shift != 0 && shift + nvalid > 64) lo |= w[1] << (64 - shift);
  return lo & mask;
}

template <int V>
__device__ __forceinline__ unsigned lane_bits(const uint8_t* __restrict__ bm, int64_t pos0, int64_t left, int lane) {
  if constexpr (V >= 8) {   // 1- and 2-byte values: 8 or 16 wave-uniform words per bitmap and step would live in scalar registers
    const int64_t mine = left - (int64_t)lane * V;   // — each lane reads its own bits, neighbours out of the same aligned words
    return (unsigned)ah_load_bits64(bm, pos0 + (int64_t)lane * V, mine >= V ? V : (int)(mine < 0 ? 0 : mine));
  }
  u64 word = 0;
#pragma unroll
  for (int w = 0; w < V; w++) {
    const u64 x = wave_bits64_const(bm, pos0 + 64 * w, left - 64 * w);
    if (((lane * V) >> 6) == w) word = x;
  }
  return (unsigned)(word >> ((lane * V) & 63)) & ((1u << V) - 1u);
}
// … of a broadcast side: its one bit for every row
template <int V>
__device__ __forceinline__ unsigned side_bits(const uint8_t* __restrict__ bm, int64_t off, bool broadcast, int64_t row0, int64_t left, int lane) {
  if (broadcast) return ah_bit(bm, off) ? (1u << V) - 1u : 0u;
  return lane_bits<V>(bm, off + row0, left, lane);
}

// W bytes per row are loaded and stored as ST words — the unsigned integer of the width, 64-bit words for 16- and 32-byte slots: the
// buffers need that alignment and no more — and selected as 32-bit words under masks made of the rows' bits
template <int W> struct CarrierOf { using type = typename UIntOf<(W < 8 ? W : 8)>::type; };
typedef unsigned Words16 __attribute__((ext_vector_type(4)));
// … 16 bytes at the alignment of ST; NT: at 16 bytes and with the nontemporal hint (a template parameter: ah_common.h says why; the
// value stays a native vector from the load to the store: taken apart and put together again, the store loses the hint)
template <int A> struct WordsAligned;
template <> struct WordsAligned<1> { typedef unsigned type __attribute__((ext_vector_type(4), aligned(1))); };
template <> struct WordsAligned<2> { typedef unsigned type __attribute__((ext_vector_type(4), aligned(2))); };
template <> struct WordsAligned<4> { typedef unsigned type __attribute__((ext_vector_type(4), aligned(4))); };
template <> struct WordsAligned<8> { typedef unsigned type __attribute__((ext_vector_type(4), aligned(8))); };
template <typename ST> using WordsAt = typename WordsAligned<(int)sizeof(ST)>::type;
template <typename ST, bool NT>
__device__ __forceinline__ Words16 load_words(const ST* p) {
  if constexpr (NT) return __builtin_nontemporal_load((const Words16*)p);
  else return *reinterpret_cast<const WordsAt<ST>*>(p);
}
template <typename ST, bool NT>
__device__ __forceinline__ void store_words(ST* p, Words16 x) {
  if constexpr (NT) __builtin_nontemporal_store(x, (Words16*)p);
  else *reinterpret_cast<WordsAt<ST>*>(p) = x;
}
// 32-bit word q (0 … 3) of a lane's 16-byte vector: all ones in the bytes of the rows whose bit is set in `bits` (bit j: row j of the step)
template <int W>
__device__ __forceinline__ unsigned word_mask(unsigned bits, int q) {
  if constexpr (W == 1) return ((((bits >> (4 * q)) & 0xFu) * 0x00204081u) & 0x01010101u) * 0xFFu;   // four rows: bit k → byte k
  else if constexpr (W == 2) return (((bits >> (2 * q)) & 1u) ? 0xFFFFu : 0u) | (((bits >> (2 * q)) & 2u) ? 0xFFFF0000u : 0u);
  else if constexpr (W == 4) return ((bits >> q) & 1u) ? ~0u : 0u;
  else if constexpr (W == 8) return ((bits >> (q >> 1)) & 1u) ? ~0u : 0u;
  else return (bits & 1u) ? ~0u : 0u;
}

template <int W, bool LB, bool RB, bool NT>
__global__ __launch_bounds__(kBlock) void if_else_kernel(const uint8_t* __restrict__ cdata, const uint8_t* __restrict__ cvalid, int64_t coff, const void* __restrict__ lv, const uint8_t* __restrict__ lvalid, int64_t loff,
                                                          const void* __restrict__ rv, const uint8_t* __restrict__ rvalid, int64_t roff, int64_t n,
                                                          void* __restrict__ outv, uint8_t* __restrict__ out_valid) {
  using ST = typename CarrierOf<W>::type;
  constexpr int EPV = 16 / (int)sizeof(ST);      // ST words per 16-byte vector
  constexpr int V = W <= 16 ? 16 / W : 1;        // rows per lane and step
  constexpr int NV = W <= 16 ? 1 : W / 16;       // vectors per lane and step
  constexpr int E = W / (int)sizeof(ST);         // ST words per row
  // row 0 of the call (a broadcast side: its one row)
  const ST* __restrict__ lp = (const ST*)lv + loff * E;
  const ST* __restrict__ rp = (const ST*)rv + roff * E;
  ST* __restrict__ op = (ST*)outv;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Words16 lb[NV], rb[NV];   // a broadcast side: its row repeated over the vector
#pragma unroll
  for (int v = 0; v < NV; v++) {
    ah_vec16<ST> x, y;
#pragma unroll
    for (int e = 0; e < EPV; e++) {
      x.v[e] = LB ? lp[(v * EPV + e) % E] : (ST)0;
      y.v[e] = RB ? rp[(v * EPV + e) % E] : (ST)0;
    }
    __builtin_memcpy(&lb[v], &x, 16);
    __builtin_memcpy(&rb[v], &y, 16);
  }
  const int64_t nsteps = (n + V - 1) / V;                               // lane steps of the column
  const int64_t ntiles = (nsteps + kBlock * kUnroll - 1) / (kBlock * kUnroll);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    Words16 lx[kUnroll][NV], rx[kUnroll][NV];
#pragma unroll
    for (int k = 0; k < kUnroll; k++) {
      const int64_t step = (tile * kUnroll + k) * kBlock + threadIdx.x;
      const bool full = (step + 1) * V <= n;
#pragma unroll
      for (int v = 0; v < NV; v++) {
        lx[k][v] = lb[v];
        rx[k][v] = rb[v];
        if (full) {
          if constexpr (!LB) lx[k][v] = load_words<ST, NT>(lp + (step * NV + v) * EPV);
          if constexpr (!RB) rx[k][v] = load_words<ST, NT>(rp + (step * NV + v) * EPV);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kUnroll; k++) {
      const int64_t wstep = (tile * kUnroll + k) * kBlock + (int64_t)wave * 64;   // the wave's first step: rows wstep · V …
      const int64_t row0 = wstep * V, left = n - row0;
      const int64_t step = wstep + lane, r0 = step * V;
      const unsigned cv = lane_bits<V>(cvalid, coff + row0, left, lane);
      const unsigned cd = lane_bits<V>(cdata, coff + row0, left, lane);
      const unsigned lok = side_bits<V>(lvalid, loff, LB, row0, left, lane);
      const unsigned rok = side_bits<V>(rvalid, roff, RB, row0, left, lane);
      const unsigned ok = cv & ((cd & lok) | (~cd & rok));   // (rows past the end: cv = 0)
      const unsigned takel = ok & cd, taker = ok & ~cd;
      if ((step + 1) * V <= n) {
        // (no loop over the NV vectors: a hinted store in a loop of one trip is rewritten by the loop passes and comes out plain)
        auto emit = [&](auto vv) {
          constexpr int v = decltype(vv)::value;
          const Words16 ml = {word_mask<W>(takel, 0), word_mask<W>(takel, 1), word_mask<W>(takel, 2), word_mask<W>(takel, 3)};
          const Words16 mr = {word_mask<W>(taker, 0), word_mask<W>(taker, 1), word_mask<W>(taker, 2), word_mask<W>(taker, 3)};
          store_words<ST, NT>(op + (step * NV + v) * EPV, (lx[k][v] & ml) | (rx[k][v] & mr));
        };
        emit(std::integral_constant<int, 0>{});
        if constexpr (NV == 2) emit(std::integral_constant<int, 1>{});
      }
      if (out_valid) {   // whole bytes: the G = 8 / V lanes of a byte fold their bits, the first of them stores
        if constexpr (V >= 8) {
#pragma unroll
          for (int b = 0; b < V / 8; b++)
            if (r0 + 8 * b < n) out_valid[(r0 >> 3) + b] = (uint8_t)(ok >> (8 * b));
        } else {
          constexpr int G = 8 / V;
          unsigned byte = ok << ((lane % G) * V);
#pragma unroll
          for (int o = 1; o < G; o <<= 1) byte |= (unsigned)__shfl_xor((int)byte, o, 64);
          if (lane % G == 0 && r0 < n) out_valid[r0 >> 3] = (uint8_t)byte;
        }
      }
    }
  }
  // the values of the column's last, partial step (n mod V rows), a row per thread.  Kept out of the loop: a plain store next to
  // a hinted one of the same address is merged with it into a plain one.
  if constexpr (V > 1) {
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < n % V) {
      const int64_t i = n - n % V + threadIdx.x;
      const bool left = ah_bit(cdata, coff + i);
      const bool ok = ah_bit(cvalid, coff + i) && (left ? ah_bit(lvalid, loff + (LB ? 0 : i)) : ah_bit(rvalid, roff + (RB ? 0 : i)));
      const ST x = LB ? lp[0] : lp[i], y = RB ? rp[0] : rp[i];   // (V > 1: one word per row)
      op[i] = ok ? (left ? x : y) : (ST)0;
    }
  }
}

// ---- ah_if_else: slots of any other width, a row per lane ---------------------------------------------------------------------------
// 0: the row is null, 1: it takes the left side, 2: the right side
__device__ __forceinline__ bool side_valid(const Side& s, int64_t i) { return ah_bit(s.valid, s.off + (s.broadcast ? 0 : i)); }
__device__ __forceinline__ int pick_side(const Cond& c, const Side& l, const Side& r, int64_t i) {
  if (!ah_bit(c.valid, c.off + i)) return 0;
  if (ah_bit(c.data, c.off + i)) return side_valid(l, i) ? 1 : 0;
  return side_valid(r, i) ? 2 : 0;
}
// the bytes of row i on side `side` (1 or 2)
__device__ __forceinline__ void side_row(int side, const Side& l, const Side& r, int64_t i, const uint8_t** p, int64_t* len) {
  if (side == 1) row_at(l.ow, l.rows, l.broadcast ? 0 : i, p, len);
  else row_at(r.ow, r.rows, r.broadcast ? 0 : i, p, len);
}

__global__ __launch_bounds__(kBlock) void if_else_bytes_kernel(Cond c, Side l, Side r, int64_t n, uint8_t* __restrict__ out, uint8_t* __restrict__ out_valid) {
  const int w = l.rows.w;
  for_wave_chunks<kBlock>(n, [&](int64_t chunk, int64_t i) {
    const int side = i < n ? pick_side(c, l, r, i) : 0;
    if (i < n) {
      const uint8_t* src = nullptr;
      int64_t len;
      if (side) side_row(side, l, r, i, &src, &len);
      uint8_t* dst = out + i * (int64_t)w;
      for (int b = 0; b < w; b++) dst[b] = side ? src[b] : (uint8_t)0;
    }
    const u64 word = __ballot(side != 0);
    if (out_valid && ah_lane() == 0) put_chunk_bytes(out_valid, chunk, n, word);
  });
}

// ---- ah_if_else_boolean ------------------------------------------------------------------------------------------------------------
// 64 bits of a side's bitmap for the rows from `row0`: a broadcast side repeats its one bit
__device__ __forceinline__ u64 side_word(const uint8_t* __restrict__ bm, int64_t off, int broadcast, int64_t row0, int cnt) {
  if (broadcast) return ah_bit(bm, off) ? (cnt >= 64 ? ~0ull : ((1ull << cnt) - 1ull)) : 0ull;
  return ah_load_bits64(bm, off + row0, cnt);
}
__global__ __launch_bounds__(kBlock) void if_else_bool_kernel(Cond c, Side l, Side r, int64_t n, uint8_t* __restrict__ out_data, uint8_t* __restrict__ out_valid) {
  const int64_t nwords = (n + 63) >> 6, stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < nwords; j += stride) {
    const int64_t row0 = j * 64;
    const int cnt = n - row0 >= 64 ? 64 : (int)(n - row0);
    const u64 cv = ah_load_bits64(c.valid, c.off + row0, cnt), cd = ah_load_bits64(c.data, c.off + row0, cnt);
    const u64 ok = cv & ((cd & side_word(l.valid, l.off, l.broadcast, row0, cnt)) | (~cd & side_word(r.valid, r.off, r.broadcast, row0, cnt)));
    const u64 d = ok & ((cd & side_word(l.rows.data, l.off, l.broadcast, row0, cnt)) | (~cd & side_word(r.rows.data, r.off, r.broadcast, row0, cnt)));
    put_chunk_bytes(out_data, j, n, d);
    if (out_valid) put_chunk_bytes(out_valid, j, n, ok);
  }
}

// ---- the var-length pair -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void if_else_lens_kernel(Cond c, Side l, Side r, int64_t n, long long* __restrict__ lens, uint8_t* __restrict__ out_valid) {
  for_wave_chunks<kBlock>(n, [&](int64_t chunk, int64_t i) {
    const int side = i < n ? pick_side(c, l, r, i) : 0;
    if (i < n) {
      const uint8_t* p;
      int64_t len = 0;
      if (side) side_row(side, l, r, i, &p, &len);
      lens[i] = len;
    }
    if (out_valid) {
      const u64 word = __ballot(side != 0);
      if (ah_lane() == 0) put_chunk_bytes(out_valid, chunk, n, word);
    }
  });
}

template <typename OffT>
__global__ __launch_bounds__(kBlock) void if_else_copy_kernel(Cond c, Side l, Side r, int64_t n, const OffT* __restrict__ out_offsets,
                                                               uint8_t* __restrict__ out_data) {
  __shared__ CopyRow s_rows[kBlock / 64][64];
  const int wave = threadIdx.x >> 6;
  for_wave_chunks<kBlock>(n, [&](int64_t, int64_t i) {
    const uint8_t* src = nullptr;
    long long dst = 0, len = 0;
    if (i < n) {
      dst = (long long)out_offsets[i];
      len = (long long)out_offsets[i + 1] - dst;
      if (len > 0) {   // ⇒ a valid row: the side is the condition's data bit
        int64_t unused;
        side_row(ah_bit(c.data, c.off + i) ? 1 : 2, l, r, i, &src, &unused);
      }
    }
    wave_copy_rows(s_rows[wave], src, out_data + dst, len);
  });
}

// ---- the directed fills ----------------------------------------------------------------------------------------------------------------
// word j of the column's validity, and its key for the carry: BACK = 0: (last valid row) + 1, BACK = 1: ~(first valid row); 0: none
__device__ __forceinline__ u64 fill_word(const uint8_t* __restrict__ valid, int64_t off, int64_t n, int64_t j) {
  const int64_t left = n - j * 64;
  return left <= 0 ? 0ull : ah_load_bits64(valid, off + j * 64, left >= 64 ? 64 : (int)left);
}
template <int BACK>
__device__ __forceinline__ unsigned word_key(u64 w, int64_t j) {
  if (!w) return 0u;
  return BACK ? ~(unsigned)(j * 64 + (__ffsll((long long)w) - 1)) : (unsigned)(j * 64 + 63 - __clzll((long long)w)) + 1u;
}

// the key of the rows of thread t's kCarryWords words folded over the workgroup: the same in every thread (one barrier)
__device__ __forceinline__ unsigned block_max(unsigned k, unsigned* s_wave) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  k = ah_wave_max(k);
  if (lane == 0) s_wave[wave] = k;
  __syncthreads();
  unsigned m = 0u;
#pragma unroll
  for (int w = 0; w < kBlock / 64; w++) m = s_wave[w] > m ? s_wave[w] : m;
  return m;
}

template <int BACK>
__global__ __launch_bounds__(kBlock) void carry_reduce_kernel(const uint8_t* __restrict__ valid, int64_t off, int64_t n, unsigned* __restrict__ block_key) {
  __shared__ unsigned s_wave[kBlock / 64];
  const int64_t j0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kCarryWords;
  unsigned k = 0u;
#pragma unroll
  for (int q = 0; q < kCarryWords; q++) {
    const unsigned kq = word_key<BACK>(fill_word(valid, off, n, j0 + q), j0 + q);
    k = kq > k ? kq : k;
  }
  k = block_max(k, s_wave);
  if (threadIdx.x == 0) block_key[blockIdx.x] = k;
}

// the exclusive running maximum of the workgroups' keys, from the left (BACK = 0) or from the right: one workgroup, each thread a
// contiguous run of keys
template <int BACK>
__global__ __launch_bounds__(kPrefixBlock) void carry_prefix_kernel(const unsigned* __restrict__ block_key, unsigned* __restrict__ block_excl, int64_t nblocks) {
  __shared__ unsigned s_wave[kPrefixBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t per = (nblocks + kPrefixBlock - 1) / kPrefixBlock;
  const int64_t lo = (int64_t)threadIdx.x * per, hi = lo + per < nblocks ? lo + per : nblocks;
  auto at = [&](int64_t q) { return BACK ? nblocks - 1 - q : q; };   // position q in scan order
  unsigned mine = 0u;
  for (int64_t q = lo; q < hi; q++) {
    const unsigned k = block_key[at(q)];
    mine = k > mine ? k : mine;
  }
  unsigned inc = mine;   // inclusive over the lanes of the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = (unsigned)__shfl_up((int)inc, o, 64);
    if (lane >= o) inc = t > inc ? t : inc;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  unsigned run = 0u;   // the waves in front, then the lanes in front
  for (int w = 0; w < wave; w++) run = s_wave[w] > run ? s_wave[w] : run;
  const unsigned before = (unsigned)__shfl_up((int)inc, 1, 64);
  if (lane > 0) run = before > run ? before : run;
  for (int64_t q = lo; q < hi; q++) {
    block_excl[at(q)] = run;
    const unsigned k = block_key[at(q)];
    run = k > run ? k : run;
  }
}

// W = 0: the indices (uint32 row numbers + validity, what Take reads); else the values gathered in the same pass
template <int W, int BACK>
__global__ __launch_bounds__(kBlock) void fill_kernel(const void* __restrict__ values_v, const uint8_t* __restrict__ valid, int64_t off, int64_t n,
                                                       const unsigned* __restrict__ block_excl, void* __restrict__ out_v, uint8_t* __restrict__ out_valid,
                                                       u64* __restrict__ valid_total) {
  constexpr int kWords = kBlock * kCarryWords;
  __shared__ u64 s_word[kWords];
  __shared__ unsigned s_carry[kWords];   // the key in front of each word (BACK: behind it)
  __shared__ unsigned s_wave[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t jb = (int64_t)blockIdx.x * kWords;          // the workgroup's first word
  // phase A: thread t owns words t·kCarryWords … of the workgroup — in scan order, so BACK walks them from the workgroup's last
  const int t = BACK ? kBlock - 1 - (int)threadIdx.x : (int)threadIdx.x;
  u64 w[kCarryWords];
  unsigned key[kCarryWords], mine = 0u;
#pragma unroll
  for (int q = 0; q < kCarryWords; q++) {
    const int64_t j = jb + t * kCarryWords + q;
    w[q] = fill_word(valid, off, n, j);
    key[q] = word_key<BACK>(w[q], j);
    mine = key[q] > mine ? key[q] : mine;
  }
  unsigned inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned x = (unsigned)__shfl_up((int)inc, o, 64);
    if (lane >= o) inc = x > inc ? x : inc;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  unsigned run = block_excl ? block_excl[blockIdx.x] : 0u;
  for (int x = 0; x < wave; x++) run = s_wave[x] > run ? s_wave[x] : run;
  const unsigned before = (unsigned)__shfl_up((int)inc, 1, 64);
  if (lane > 0) run = before > run ? before : run;
  unsigned nvalid = 0u;
#pragma unroll
  for (int qq = 0; qq < kCarryWords; qq++) {
    const int q = BACK ? kCarryWords - 1 - qq : qq;   // scan order inside the thread
    const int jl = t * kCarryWords + q;
    s_word[jl] = w[q];
    s_carry[jl] = run;
    // the word's output validity: every row once a source lies in front (behind), else from the word's first (up to its last) valid row
    const int64_t left = n - (jb + jl) * 64;
    if (left > 0) {
      u64 ov = run ? ~0ull : (w[q] ? (BACK ? ~0ull >> __clzll((long long)w[q]) : ~0ull << (__ffsll((long long)w[q]) - 1)) : 0ull);
      if (left < 64) ov &= (1ull << left) - 1ull;
      nvalid += (unsigned)__popcll(ov);
      if (out_valid) put_chunk_bytes(out_valid, jb + jl, n, ov);
    }
    run = key[q] > run ? key[q] : run;
  }
  if (valid_total) {
    nvalid = ah_wave_sum(nvalid);
    if (lane == 0 && nvalid) atomicAdd(valid_total, (u64)nvalid);
  }
  __syncthreads();
  // phase B: the workgroup's rows in coalesced order, V rows per lane and step
  using ST = typename CarrierOf<(W ? W : 4)>::type;
  constexpr int WB = W ? W : 4;
  constexpr int V = WB <= 16 ? 16 / WB : 1, NV = WB <= 16 ? 1 : WB / 16, E = WB / (int)sizeof(ST), EPV = 16 / (int)sizeof(ST);
  const ST* __restrict__ vals = W ? (const ST*)values_v + off * E : nullptr;   // row 0 of the call
  ST* __restrict__ op = (ST*)out_v;
  const int64_t rb = jb * 64;
  const int64_t rows = n - rb < kCarryRows ? n - rb : kCarryRows;
  for (int64_t s = threadIdx.x; s * V < rows; s += kBlock) {
    const int64_t r0 = rb + s * V;
    ah_vec16<ST> o[NV];
    const bool full = r0 + V <= n;
    const int jl = (int)((s * V) >> 6), b0 = (int)((s * V) & 63);
    const u64 word = s_word[jl];
    const unsigned carry = s_carry[jl];
    const unsigned own = (unsigned)(word >> b0) & ((1u << V) - 1u);
    if constexpr (W != 0) {
      if (full && own == (1u << V) - 1u) {   // every row of the step is its own source: the vector as it is
#pragma unroll
        for (int v = 0; v < NV; v++) ah_st16<ST>(op + (r0 * E + v * EPV), ah_ld16<ST>(vals + (r0 * E + v * EPV)));
        continue;
      }
    }
#pragma unroll
    for (int j = 0; j < V; j++) {
      const int b = b0 + j;
      const u64 m = BACK ? word & (~0ull << b) : word & (~0ull >> (63 - b));
      bool ok = true;
      unsigned src;
      if (m) src = (unsigned)(rb + jl * 64 + (BACK ? __ffsll((long long)m) - 1 : 63 - __clzll((long long)m)));
      else { ok = carry != 0u; src = BACK ? ~carry : carry - 1u; }
      ok = ok && r0 + j < n;
      if constexpr (W == 0) {
        o[0].v[j] = ok ? src : 0u;
      } else {
#pragma unroll
        for (int e = 0; e < E; e++) {
          const ST x = ok ? vals[(int64_t)src * E + e] : (ST)0;
          o[(j * E + e) / EPV].v[(j * E + e) % EPV] = x;
        }
      }
    }
    if (full) {
#pragma unroll
      for (int v = 0; v < NV; v++) ah_st16<ST>(op + (r0 * E + v * EPV), o[v]);
    } else {   // the column's last, partial step (compile-time indices: the vectors stay in registers)
#pragma unroll
      for (int j = 0; j < V; j++)
#pragma unroll
        for (int e = 0; e < E; e++)
          if (r0 + j < n) op[(r0 + j) * E + e] = o[(j * E + e) / EPV].v[(j * E + e) % EPV];
    }
  }
}

template <int W, int BACK>
int run_fill_dir(ah_ctx* c, const void* values, const uint8_t* valid, int64_t off, int64_t n, void* out, uint8_t* out_valid, u64* valid_total) {
  const int64_t nblocks = ah_ceil_div(n, kCarryRows);
  unsigned *block_key = nullptr, *block_excl = nullptr;
  if (nblocks > 1) {
    auto carve = [&](TempCarver& t) {
      t.take(block_key, (size_t)nblocks);
      t.take(block_excl, (size_t)nblocks);
    };
    TempCarver measure;
    carve(measure);
    TempCarver block;
    int rc = ah_scratch_reserve(c, measure.used, (void**)&block.base);
    if (rc != AH_OK) return rc;
    carve(block);
    carry_reduce_kernel<BACK><<<(unsigned)nblocks, kBlock, 0, c->stream>>>(valid, off, n, block_key);
    AH_LAUNCH_CHECK(c);
    carry_prefix_kernel<BACK><<<1, kPrefixBlock, 0, c->stream>>>(block_key, block_excl, nblocks);
    AH_LAUNCH_CHECK(c);
  }
  fill_kernel<W, BACK><<<(unsigned)nblocks, kBlock, 0, c->stream>>>(values, valid, off, n, block_excl, out, out_valid, valid_total);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

// both entries: the checks, the launches, and the null count home when the caller asks for it (the one synchronisation)
int run_fill(ah_ctx* c, const char* fn, int byte_width, const void* values, const uint8_t* valid, int64_t off, int64_t n, int direction, void* out,
             uint8_t* out_valid, int64_t* out_null_count_host) {
  if (out_null_count_host) *out_null_count_host = 0;
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "%s: negative length/offset", fn);
  if (direction != 0 && direction != 1) return ah_fail(c, AH_EINVALID, "%s: direction %d is neither 0 (forward) nor 1 (backward)", fn, direction);
  if (n > kFillMaxRows) return ah_fail(c, AH_ENOTIMPL, "%s: %lld rows, more than 2^32 - 1", fn, (long long)n);
  if (n == 0) return AH_OK;
  if (!out || (byte_width && !values)) return ah_fail(c, AH_EINVALID, "%s: null buffer", fn);
  if (valid && !out_valid) return ah_fail(c, AH_EINVALID, "%s: a column with a validity bitmap needs an output bitmap", fn);
  const int align = byte_width == 0 ? 4 : byte_width < 8 ? byte_width : 8;
  if (((uintptr_t)out | (uintptr_t)values) & (uintptr_t)(align - 1)) return ah_fail(c, AH_EINVALID, "%s: buffer not element-aligned", fn);
  u64* total = out_null_count_host ? (u64*)&c->dscalars[2] : nullptr;
  if (total) AH_HIP(c, hipMemsetAsync(total, 0, sizeof(u64), c->stream));
  int rc = AH_OK;
  const bool known = with_value_width<0, 1, 2, 4, 8, 16, 32>(byte_width, [&](auto w) {
    constexpr int W = decltype(w)::value;
    rc = direction ? run_fill_dir<W, 1>(c, values, valid, off, n, out, out_valid, total) : run_fill_dir<W, 0>(c, values, valid, off, n, out, out_valid, total);
  });
  if (!known) return ah_fail(c, AH_ENOTIMPL, "%s: values of %d bytes", fn, byte_width);
  if (rc != AH_OK) return rc;
  if (total) {
    AH_HIP(c, hipMemcpyAsync(c->pinned, total, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    AH_HIP(c, hipStreamSynchronize(c->stream));
    *out_null_count_host = n - (int64_t) * (volatile uint64_t*)&c->pinned[0];
  }
  return AH_OK;
}

// ---- host side of if_else ---------------------------------------------------------------------------------------------------------------
int check_if_else(ah_ctx* c, const char* fn, const uint8_t* cond_data, int64_t cond_off, const ah_cond_side* l, const ah_cond_side* r, int64_t n) {
  if (n < 0 || cond_off < 0) return ah_fail(c, AH_EINVALID, "%s: negative length/offset", fn);
  if (!l || !r) return ah_fail(c, AH_EINVALID, "%s: null side", fn);
  if (l->off < 0 || r->off < 0) return ah_fail(c, AH_EINVALID, "%s: negative side offset", fn);
  if (n > 0 && !cond_data) return ah_fail(c, AH_EINVALID, "%s: null condition", fn);
  return AH_OK;
}
Side side_of(const ah_cond_side& s) {
  return Side{byte_rows(s.offset_width, s.offsets, (const uint8_t*)s.data, s.byte_width, s.off), s.offset_width, s.valid, s.off, s.broadcast ? 1 : 0};
}

template <int W>
int launch_if_else(ah_ctx* c, const Cond& cond, const ah_cond_side& l, const ah_cond_side& r, int64_t n, void* out, uint8_t* out_valid) {
  constexpr int V = W <= 16 ? 16 / W : 1;
  const uintptr_t la = l.broadcast ? 0 : (uintptr_t)l.data + (uintptr_t)l.off * W, ra = r.broadcast ? 0 : (uintptr_t)r.data + (uintptr_t)r.off * W;
  const bool nt = c->tune_nt && ((la | ra | (uintptr_t)out) & 15) == 0;
  const unsigned grid = ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, V), (int64_t)kBlock * kUnroll), /*default_bpc=*/0);
#define AH_IF_ELSE(LB, RB)                                                                                                                       \
  do {                                                                                                                                           \
    if (nt) if_else_kernel<W, LB, RB, true><<<grid, kBlock, 0, c->stream>>>(cond.data, cond.valid, cond.off, l.data, l.valid, l.off, r.data, r.valid, r.off, n, out, out_valid);  \
    else if_else_kernel<W, LB, RB, false><<<grid, kBlock, 0, c->stream>>>(cond.data, cond.valid, cond.off, l.data, l.valid, l.off, r.data, r.valid, r.off, n, out, out_valid);    \
  } while (0)
  if (l.broadcast && r.broadcast) AH_IF_ELSE(true, true);
  else if (l.broadcast) AH_IF_ELSE(true, false);
  else if (r.broadcast) AH_IF_ELSE(false, true);
  else AH_IF_ELSE(false, false);
#undef AH_IF_ELSE
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

}  // namespace

AH_EXPORT int ah_if_else(ah_ctx* c, const uint8_t* cond_data, const uint8_t* cond_valid, int64_t cond_off, const ah_cond_side* l,
                         const ah_cond_side* r, int64_t n, void* out_values, uint8_t* out_valid) {
  AH_ENTER(c);
  int rc = check_if_else(c, "if_else", cond_data, cond_off, l, r, n);
  if (rc != AH_OK) return rc;
  if (l->offset_width || r->offset_width) return ah_fail(c, AH_EINVALID, "if_else: a var-length side (ah_if_else_binary_offsets / _data take those)");
  const int w = l->byte_width;
  if (w != r->byte_width) return ah_fail(c, AH_EINVALID, "if_else: sides of %d and %d bytes", w, r->byte_width);
  if (w < 1 || w > 4096) return ah_fail(c, AH_EINVALID, "if_else: byte width %d (1 … 4096)", w);
  if (n == 0) return AH_OK;
  if (!l->data || !r->data || !out_values) return ah_fail(c, AH_EINVALID, "if_else: null buffer");
  if (!out_valid && (cond_valid || l->valid || r->valid)) return ah_fail(c, AH_EINVALID, "if_else: an input with a validity bitmap needs an output bitmap");
  const Cond cond{cond_data, cond_valid, cond_off};
  // the vector path moves words of the slot's width (8 bytes for 16- and 32-byte slots): buffers aligned to less take the rows' path
  const uintptr_t word = (uintptr_t)(w < 8 ? w : 8) - 1;
  const bool misaligned = (((uintptr_t)l->data | (uintptr_t)r->data | (uintptr_t)out_values) & word) != 0;
  const bool slot = with_value_width<1, 2, 4, 8, 16, 32>(misaligned ? 0 : w, [&](auto ww) { rc = launch_if_else<decltype(ww)::value>(c, cond, *l, *r, n, out_values, out_valid); });
  if (slot) return rc;
  if_else_bytes_kernel<<<ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, 64), kBlock / 64), 8), kBlock, 0, c->stream>>>(cond, side_of(*l), side_of(*r), n,
                                                                                                                   (uint8_t*)out_values, out_valid);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

AH_EXPORT int ah_if_else_boolean(ah_ctx* c, const uint8_t* cond_data, const uint8_t* cond_valid, int64_t cond_off, const ah_cond_side* l,
                                 const ah_cond_side* r, int64_t n, uint8_t* out_data, uint8_t* out_valid) {
  AH_ENTER(c);
  int rc = check_if_else(c, "if_else_boolean", cond_data, cond_off, l, r, n);
  if (rc != AH_OK) return rc;
  if (n == 0) return AH_OK;
  if (!l->data || !r->data || !out_data) return ah_fail(c, AH_EINVALID, "if_else_boolean: null buffer");
  if (!out_valid && (cond_valid || l->valid || r->valid))
    return ah_fail(c, AH_EINVALID, "if_else_boolean: an input with a validity bitmap needs an output bitmap");
  // a side's data is a bitmap read at bit off + row, like its validity
  const Side ls{ByteRows{nullptr, (const uint8_t*)l->data, 0}, 0, l->valid, l->off, l->broadcast ? 1 : 0};
  const Side rs{ByteRows{nullptr, (const uint8_t*)r->data, 0}, 0, r->valid, r->off, r->broadcast ? 1 : 0};
  if_else_bool_kernel<<<ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, 64), kBlock), 8), kBlock, 0, c->stream>>>(Cond{cond_data, cond_valid, cond_off}, ls, rs, n,
                                                                                                             out_data, out_valid);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

AH_EXPORT int ah_if_else_binary_offsets(ah_ctx* c, const uint8_t* cond_data, const uint8_t* cond_valid, int64_t cond_off, const ah_cond_side* l,
                                        const ah_cond_side* r, int64_t n, int out_offset_width, void* out_offsets, uint8_t* out_valid,
                                        int64_t* out_total_bytes_host) {
  AH_ENTER(c);
  if (out_total_bytes_host) *out_total_bytes_host = 0;
  int rc = check_if_else(c, "if_else_binary", cond_data, cond_off, l, r, n);
  if (rc != AH_OK) return rc;
  for (const ah_cond_side* s : {l, r}) {
    if (s->offset_width != 4 && s->offset_width != 8) return ah_fail(c, AH_EINVALID, "if_else_binary: binary offsets are 4 or 8 bytes wide");
    if (!s->offsets) return ah_fail(c, AH_EINVALID, "if_else_binary: null buffer");
  }
  if (out_offset_width != 4 && out_offset_width != 8) return ah_fail(c, AH_EINVALID, "if_else_binary: binary offsets are 4 or 8 bytes wide");
  if (!out_offsets) return ah_fail(c, AH_EINVALID, "if_else_binary: null buffer");
  if (!out_valid && (cond_valid || l->valid || r->valid))
    return ah_fail(c, AH_EINVALID, "if_else_binary: an input with a validity bitmap needs an output bitmap");
  if (n == 0) {   // a lone closing offset
    AH_HIP(c, hipMemsetAsync(out_offsets, 0, (size_t)out_offset_width, c->stream));
    return AH_OK;
  }
  VarOut v;
  rc = varout_begin(c, n, 0, /*can_overflow=*/true, &v);
  if (rc != AH_OK) return rc;
  if_else_lens_kernel<<<ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, 64), kBlock / 64), 8), kBlock, 0, c->stream>>>(Cond{cond_data, cond_valid, cond_off}, side_of(*l),
                                                                                                                    side_of(*r), n, v.lens, out_valid);
  AH_LAUNCH_CHECK(c);
  rc = varout_enqueue(c, v, n, out_offset_width, out_offsets, /*caller_words=*/false);
  if (rc != AH_OK) return rc;
  int64_t total = 0;
  bool overflow = false;
  rc = varout_finish(c, v, &total, &overflow);
  if (rc != AH_OK) return rc;
  if (overflow) return ah_fail(c, AH_EINVALID, "binary output offset overflow");
  if (out_total_bytes_host) *out_total_bytes_host = total;
  return AH_OK;
}

AH_EXPORT int ah_if_else_binary_data(ah_ctx* c, const uint8_t* cond_data, const uint8_t* cond_valid, int64_t cond_off, const ah_cond_side* l,
                                     const ah_cond_side* r, int64_t n, int out_offset_width, const void* out_offsets, uint8_t* out_data) {
  AH_ENTER(c);
  int rc = check_if_else(c, "if_else_binary", cond_data, cond_off, l, r, n);
  if (rc != AH_OK) return rc;
  for (const ah_cond_side* s : {l, r}) {
    if (s->offset_width != 4 && s->offset_width != 8) return ah_fail(c, AH_EINVALID, "if_else_binary: binary offsets are 4 or 8 bytes wide");
    if (!s->offsets) return ah_fail(c, AH_EINVALID, "if_else_binary: null buffer");
  }
  if (out_offset_width != 4 && out_offset_width != 8) return ah_fail(c, AH_EINVALID, "if_else_binary: binary offsets are 4 or 8 bytes wide");
  if (n == 0) return AH_OK;
  if (!out_offsets) return ah_fail(c, AH_EINVALID, "if_else_binary: null buffer");
  (void)cond_valid;   // a null row has length 0 in out_offsets: nothing of it is copied
  const Cond cond{cond_data, nullptr, cond_off};
  const unsigned grid = ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, 64), kBlock / 64), 16);
  if (out_offset_width == 4) if_else_copy_kernel<int32_t><<<grid, kBlock, 0, c->stream>>>(cond, side_of(*l), side_of(*r), n, (const int32_t*)out_offsets, out_data);
  else if_else_copy_kernel<int64_t><<<grid, kBlock, 0, c->stream>>>(cond, side_of(*l), side_of(*r), n, (const int64_t*)out_offsets, out_data);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

AH_EXPORT int ah_fill_null_indices(ah_ctx* c, const uint8_t* valid, int64_t off, int64_t n, int direction, uint32_t* out_idx, uint8_t* out_idx_valid,
                                   int64_t* out_null_count_host) {
  AH_ENTER(c);
  return run_fill(c, "fill_null_indices", 0, nullptr, valid, off, n, direction, out_idx, out_idx_valid, out_null_count_host);
}

AH_EXPORT int ah_fill_null_directed(ah_ctx* c, int byte_width, const void* values, const uint8_t* valid, int64_t off, int64_t n, int direction,
                                    void* out_values, uint8_t* out_valid, int64_t* out_null_count_host) {
  AH_ENTER(c);
  if (!with_value_width<1, 2, 4, 8, 16, 32>(byte_width, [](auto) {}))
    return ah_fail(c, AH_ENOTIMPL, "fill_null_directed: values of %d bytes (1, 2, 4, 8, 16 or 32; any other width: ah_fill_null_indices and a Take)", byte_width);
  return run_fill(c, "fill_null_directed", byte_width, values, valid, off, n, direction, out_values, out_valid, out_null_count_host);
}
