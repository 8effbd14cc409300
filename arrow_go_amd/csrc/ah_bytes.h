// ah_bytes.h — the byte-row layer of the String / Binary / LargeString / LargeBinary, FixedSizeBinary and Decimal kernels:
// ah_hash.hip (unique / dictionary_encode), ah_setlookup_binary.hip (is_in), ah_compare_binary.hip (comparisons) and
// ah_sort_binary.hip (sort_indices).  Where row i's bytes are (ByteRows / row_at), unaligned 8-byte loads, the 64-bit hash of a
// byte string, byte equality, the unsigned bytewise order (bytes.Compare), and the whole-wave compare of long values.
#pragma once
#include "ah_common.h"

namespace {

// A column of byte rows, its pointers of row 0 of the call (the array offset already applied): 4- or 8-byte offsets into
// `data`, or fixed slots of `w` bytes from `data`.  The offset width selects the layout: OW = 4, 8, or 0 for fixed width.
struct ByteRows {
  const void* offsets;
  const uint8_t* data;
  int w;
};

// the column of a buffer pair and an array offset (offsets of entry `off`, or slot `off`)
inline ByteRows byte_rows(int ow, const void* offsets, const uint8_t* data, int w, int64_t off) {
  if (ow == 4) return ByteRows{(const int32_t*)offsets + off, data, w};
  if (ow == 8) return ByteRows{(const long long*)offsets + off, data, w};
  return ByteRows{nullptr, data + off * (int64_t)w, w};
}

// row i: its first byte and its length
template <int OW>
__device__ __forceinline__ void row_at(const ByteRows& c, int64_t i, const uint8_t** p, int64_t* len) {
  if constexpr (OW == 4) {
    const int64_t b = ((const int32_t*)c.offsets)[i], e = ((const int32_t*)c.offsets)[i + 1];
    *p = c.data + b;
    *len = e - b;
  } else if constexpr (OW == 8) {
    const int64_t b = ((const long long*)c.offsets)[i], e = ((const long long*)c.offsets)[i + 1];
    *p = c.data + b;
    *len = e - b;
  } else {
    *p = c.data + i * (int64_t)c.w;
    *len = c.w;
  }
}
// … with the layout chosen at run time
__device__ __forceinline__ void row_at(int ow, const ByteRows& c, int64_t i, const uint8_t** p, int64_t* len) {
  if (ow == 4) row_at<4>(c, i, p, len);
  else if (ow == 8) row_at<8>(c, i, p, len);
  else row_at<0>(c, i, p, len);
}

struct U64u { unsigned long long v; } __attribute__((packed, aligned(1)));
__device__ __forceinline__ unsigned long long load8(const uint8_t* p) { return reinterpret_cast<const U64u*>(p)->v; }
__device__ __forceinline__ unsigned long long load_tail(const uint8_t* p, int nb) {  // 1..7 bytes, little-endian
  unsigned long long w = 0;
  for (int t = 0; t < nb; t++) w |= (unsigned long long)p[t] << (8 * t);
  return w;
}
// Any 64-bit hash will do: ids and dictionary order depend only on which rows are EQUAL and on row order,
// never on hash values (the reference's xxh3 / custom short-string hash, hash_funcs.go:86-124, decides
// only where its own memo table stores an entry).  Multiply-xorshift over 8-byte words.
__device__ __forceinline__ uint64_t hash_bytes(const uint8_t* p, int64_t len) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ ((uint64_t)len * 0xC2B2AE3D27D4EB4Full);
  int64_t j = 0;
  for (; j + 8 <= len; j += 8) {
    h = (h ^ load8(p + j)) * 0xFF51AFD7ED558CCDull;
    h ^= h >> 32;
  }
  if (j < len) {
    h = (h ^ load_tail(p + j, (int)(len - j))) * 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 29;
  }
  h *= 0x9FB21C651E98DF25ull;
  return h ^ (h >> 32);
}
__device__ __forceinline__ bool equal_bytes(const uint8_t* a, const uint8_t* b, int64_t len) {
  int64_t j = 0;
  for (; j + 8 <= len; j += 8)
    if (load8(a + j) != load8(b + j)) return false;
  return j == len || load_tail(a + j, (int)(len - j)) == load_tail(b + j, (int)(len - j));
}

// bytes.Compare of two little-endian loads of the same bytes: −1 / 0 / 1
__device__ __forceinline__ int order_words(unsigned long long x, unsigned long long y) {
  if (x == y) return 0;
  return __builtin_bswap64(x) < __builtin_bswap64(y) ? -1 : 1;
}

// bytes.Compare of bytes [from, to) of a and b (both at least `to` long): −1 / 0 / 1.  `from` is a multiple of 8, so a
// value staged in LDS is read in aligned words.
__device__ __forceinline__ int order_range(const uint8_t* a, const uint8_t* b, int64_t from, int64_t to) {
  int64_t j = from;
  for (; j + 8 <= to; j += 8) {
    const int c = order_words(load8(a + j), load8(b + j));
    if (c) return c;
  }
  if (j < to) return order_words(load_tail(a + j, (int)(to - j)), load_tail(b + j, (int)(to - j)));
  return 0;
}

// the 8 bytes at p + j of a value `len` bytes long, zero-padded past its end (j < len)
__device__ __forceinline__ unsigned long long word_at(const uint8_t* p, int64_t j, int64_t len) {
  return len - j >= 8 ? load8(p + j) : load_tail(p + j, (int)(len - j));
}

// The wave takes the lanes in `need` (wave-uniform; called with all 64 lanes active), one after another: body(l) with the number of
// the lane whose turn it is — every lane runs it, for lane l's row, whose values it fetches with __shfl(x, l).
template <typename Body>
__device__ __forceinline__ void for_pending_lanes(unsigned long long need, Body body) {
  while (need) {
    const int l = __ffsll((long long)need) - 1;
    need &= need - 1;
    body(l);
  }
}

// The whole wave compares the long values of the lanes in `need` (wave-uniform; called with all 64 lanes active), one
// pending lane after another, 512 bytes per step (64 lanes × 8 bytes): bytes [from, len) of a and b, `from` a multiple of 8.
// Each pending lane then calls done(r) with the result for its own a, b, len:
//   ORDER:  bytes.Compare of the range, −1 / 0 / 1, stopping at the first step that differs (one ballot per step);
//   !ORDER: 0 when the ranges are equal, else 1 (one ballot per value).
// The callback updates the caller's own state in place; a returned per-lane result cost the is_in probe 2-4 VGPRs.
template <bool ORDER, typename Done>
__device__ __forceinline__ void wave_compare(unsigned long long need, const uint8_t* a, const uint8_t* b, int64_t len, int64_t from, Done done) {
  const int lane = ah_lane();
  for_pending_lanes(need, [&](int l) {
    const uint8_t* wa = (const uint8_t*)(uintptr_t)__shfl((long long)(uintptr_t)a, l);
    const uint8_t* wb = (const uint8_t*)(uintptr_t)__shfl((long long)(uintptr_t)b, l);
    const int64_t m = __shfl((long long)len, l);
    int r = 0;
    if constexpr (ORDER) {
      for (int64_t base = from; base < m; base += 64 * 8) {
        const int64_t j = base + (int64_t)lane * 8;
        const int c = j < m ? order_words(word_at(wa, j, m), word_at(wb, j, m)) : 0;
        const unsigned long long d = __ballot(c != 0);
        if (d) {
          r = __shfl(c, __ffsll((long long)d) - 1);
          break;
        }
      }
    } else {
      bool diff = false;
      for (int64_t j = from + (int64_t)lane * 8; j < m; j += 64 * 8) diff |= word_at(wa, j, m) != word_at(wb, j, m);
      r = __ballot(diff) != 0ull;
    }
    if (lane == l) done(r);
  });
}

// The row copy of the var-length outputs (the Take of ah_varlen.hip, the if_else of ah_conditional.hip): a wave owns 64 output rows,
// each lane brings its row's source, destination and length (len ≤ 0: nothing to copy).  The rows that have bytes are compacted
// into `s_rows` (the wave's own 64 entries of LDS) in row order; four 16-lane groups then copy four rows at a time, 4 (unaligned)
// bytes per lane.  Called with all 64 lanes active; s_rows may be reused as soon as it returns.
struct CopyRow { const uint8_t* src; uint8_t* dst; long long len; };
struct __attribute__((packed)) U32u { unsigned v; };  // 4 bytes at any address (gfx950 global memory runs in unaligned-access mode)
__device__ __forceinline__ void wave_copy_rows(CopyRow* s_rows, const uint8_t* src, uint8_t* dst, long long len) {
  const int lane = ah_lane();
  const int group = lane >> 4, sub = lane & 15;
  const unsigned long long todo = __ballot(len > 0);
  const int count = __popcll(todo);
  if (len > 0) s_rows[__popcll(todo & (lane == 0 ? 0ull : (~0ull >> (64 - lane))))] = CopyRow{src, dst, len};
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // LDS ops of a wave are in order; keep the compiler from reordering
  __builtin_amdgcn_wave_barrier();
  for (int k = group; k < count; k += 4) {
    volatile const CopyRow* rp = &s_rows[k];  // written by other lanes of this wave
    CopyRow r;
    r.src = rp->src; r.dst = rp->dst; r.len = rp->len;
    long long b = (long long)sub * 4;
    for (; b + 4 <= r.len; b += 64) ((U32u*)(r.dst + b))->v = ((const U32u*)(r.src + b))->v;
    const long long tail = r.len & ~3ll;  // the last len mod 4 bytes
    if (sub < (int)(r.len - tail)) r.dst[tail + sub] = r.src[tail + sub];
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the next chunk overwrites s_rows
  __builtin_amdgcn_wave_barrier();
}

}  // namespace
