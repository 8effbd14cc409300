// ah_lz4.h — one LZ4 block decoded by a group of cooperating lanes.  Compiled for the device (ah_lz4.hip: the 64
// lanes of a wavefront) and for the host (tests/lz4_harness.cc: lanes 0 … 63 in a loop) from the same text: the sequence parsing,
// every bounds decision and the address arithmetic of every copy loop are this file's, only `Par` — how "all lanes do f" and "all
// lanes have done it" are spelt — differs.
//
//   Par::lanes(f)   every lane runs f(lane, nlanes); when it returns, what the lanes wrote is visible to all of them
//   Par::sync()     what the lanes read before it is read before anything after it is written
//   Par::uni(x)     x, which is the same in every lane, as a value the compiler may keep in a scalar register
//
// The block format (lz4_Block_format.md): sequences of {token, [literal length bytes], literals, offset (u16 LE), [match length
// bytes]}; the last sequence ends after its literals.  The output image and the input window are the caller's memory (LDS on the
// device).  A match reads the image only below the position it starts at — byte i of a match is image[pos − offset + (i mod offset)]
// — so the lanes of one copy never depend on each other, and consecutive copies are separated by lanes()'s visibility.
//
// A corrupt block becomes a status, never a fault: every source index is checked against the block's end, every output index against
// dst_len, an offset must satisfy 1 ≤ offset ≤ bytes produced so far, the length-extension loops stop at the source end (and at the
// first length no 64 KiB block can hold).  The encoder-side end-of-block rules (last five bytes literal, …) are not enforced, as
// liblz4's decoder does not enforce them.  Nothing here waits for anything: a block's decode is a bounded loop over its own bytes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AH_LZ4_HD __host__ __device__ __forceinline__
#else
#define AH_LZ4_HD inline __attribute__((always_inline))
#endif

enum : int { AH_LZ4_OK = 0, AH_LZ4_CORRUPT = 1, AH_LZ4_WRONG_SIZE = 2 };
constexpr uint32_t kLz4MaxBlock = 65536;   // bytes of output image: the largest dst_len
constexpr uint32_t kLz4Window = 4096;      // bytes of input window (a multiple of 16)
constexpr uint32_t kLz4MaxSrc = 1u << 30;  // positions are 32-bit: a longer source is refused before the decode

// 16 bytes between two 16-byte aligned addresses: one vector load and one vector store (a copy of bytes, so no aliasing question)
AH_LZ4_HD void ah_lz4_move16(uint8_t* to, const uint8_t* from) {
  __builtin_memcpy(__builtin_assume_aligned(to, 16), __builtin_assume_aligned(from, 16), 16);
}

// ---- the copy loops: (lane, nlanes) → the bytes that lane moves ------------------------------------------------------------------
// Window := block bytes [wv − mis, wv − mis + kLz4Window) ∩ [0, slen).  Positions are "virtual": block position + mis, where mis is
// the block's misalignment in memory, so a virtual multiple of 16 is a 16-byte aligned address.  A 16-byte slot that lies inside the
// block is one aligned 16-byte load; a slot that straddles either end of the block is read byte by byte, inside the block only.
AH_LZ4_HD void ah_lz4_refill(uint8_t* win, const uint8_t* src, uint32_t slen, uint32_t mis, uint32_t wv, int lane, int nlanes) {
  for (uint32_t j = (uint32_t)lane; j < kLz4Window / 16; j += (uint32_t)nlanes) {
    const int64_t b0 = (int64_t)wv + 16 * (int64_t)j - (int64_t)mis;   // block position of the slot's first byte
    if (b0 >= (int64_t)slen) break;
    if (b0 >= 0 && b0 + 16 <= (int64_t)slen) {
      ah_lz4_move16(win + 16 * j, src + b0);
    } else {
      for (int k = 0; k < 16; k++) {
        const int64_t b = b0 + k;
        if (b >= 0 && b < (int64_t)slen) win[16 * j + k] = src[b];
      }
    }
  }
}
AH_LZ4_HD void ah_lz4_copy_literals(uint8_t* dst, const uint8_t* from, uint32_t n, int lane, int nlanes) {
  for (uint32_t i = (uint32_t)lane; i < n; i += (uint32_t)nlanes) dst[i] = from[i];
}
// n bytes at image[pos …] := the match `offset` bytes back, 1 ≤ offset ≤ pos
AH_LZ4_HD void ah_lz4_copy_match(uint8_t* image, uint32_t pos, uint32_t offset, uint32_t n, int lane, int nlanes) {
  const uint8_t* from = image + (pos - offset);
  uint8_t* to = image + pos;
  if (offset >= n) {
    for (uint32_t i = (uint32_t)lane; i < n; i += (uint32_t)nlanes) to[i] = from[i];
  } else {   // the match runs into its own output: the pattern of `offset` bytes repeats; i mod offset without a division per byte
    uint32_t r = (uint32_t)lane % offset;
    const uint32_t step = (uint32_t)nlanes % offset;
    for (uint32_t i = (uint32_t)lane; i < n; i += (uint32_t)nlanes) {
      to[i] = from[r];
      r += step;
      if (r >= offset) r -= offset;
    }
  }
}
// the finished image → its place in the output: 16 bytes per lane and step where the destination is 16-byte aligned
AH_LZ4_HD void ah_lz4_flush(uint8_t* dst, const uint8_t* image, uint32_t n, int lane, int nlanes) {
  uint32_t done = 0;
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const uint32_t nvec = n / 16;
    for (uint32_t j = (uint32_t)lane; j < nvec; j += (uint32_t)nlanes)
      ah_lz4_move16(dst + 16 * j, image + 16 * j);
    done = nvec * 16;
  }
  for (uint32_t i = done + (uint32_t)lane; i < n; i += (uint32_t)nlanes) dst[i] = image[i];
}

// ---- the sequencer: the same in every lane -------------------------------------------------------------------------------------
template <class Par>
struct ah_lz4_decoder {
  Par& par;
  const uint8_t* src;   // the block's first byte
  uint32_t slen;
  uint8_t* image;       // ≥ dlen bytes, 16-byte aligned
  uint32_t dlen;
  uint8_t* win;         // kLz4Window bytes, 16-byte aligned
  uint32_t mis, wv;     // see ah_lz4_refill

  // the window holds block bytes [p, p + need) afterwards; the caller has checked p + need ≤ slen
  AH_LZ4_HD void ensure(uint32_t p, uint32_t need) {
    const uint32_t v = p + mis;
    if (v + need <= wv + kLz4Window) return;   // (v ≥ wv always: positions only grow)
    wv = v & ~15u;
    par.sync();
    const uint8_t* s = src;
    uint8_t* w = win;
    const uint32_t sl = slen, m = mis, base = wv;
    par.lanes([=](int lane, int nlanes) { ah_lz4_refill(w, s, sl, m, base, lane, nlanes); });
  }
  AH_LZ4_HD uint32_t byte_at(uint32_t p) {
    ensure(p, 1);
    return par.uni((uint32_t)win[p + mis - wv]);
  }
  // literals: n source bytes from position sp → image[op …]; the caller has checked n ≤ slen − sp and n ≤ dlen − op
  AH_LZ4_HD void literals(uint32_t sp, uint32_t op, uint32_t n) {
    while (n) {
      ensure(sp, 1);
      const uint32_t at = sp + mis - wv, room = kLz4Window - at;
      const uint32_t m = n < room ? n : room;
      uint8_t* to = image + op;
      const uint8_t* from = win + at;
      par.lanes([=](int lane, int nlanes) { ah_lz4_copy_literals(to, from, m, lane, nlanes); });
      sp += m; op += m; n -= m;
    }
  }
  // token nibble 15: add bytes until one is not 255.  false: the source ended, or the length is beyond any block.
  AH_LZ4_HD bool extend(uint32_t* sp, uint32_t* len) {
    for (;;) {
      if (*sp >= slen) return false;
      const uint32_t b = byte_at((*sp)++);
      *len += b;
      if (*len > kLz4MaxBlock) return false;
      if (b != 255) return true;
    }
  }

  AH_LZ4_HD int run(bool stored) {
    if (dlen > kLz4MaxBlock || slen > kLz4MaxSrc) return AH_LZ4_CORRUPT;
    mis = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15);
    wv = 0;
    if (slen > 0) {
      par.sync();                 // the window starts at the 16-byte line that holds the block's first byte
      const uint8_t* s = src;
      uint8_t* w = win;
      const uint32_t sl = slen, m = mis;
      par.lanes([=](int lane, int nlanes) { ah_lz4_refill(w, s, sl, m, 0u, lane, nlanes); });
    }
    if (stored) {
      if (slen > dlen) return AH_LZ4_CORRUPT;
      literals(0, 0, slen);
      return slen == dlen ? AH_LZ4_OK : AH_LZ4_WRONG_SIZE;
    }
    uint32_t sp = 0, op = 0;
    for (;;) {
      if (sp >= slen) return AH_LZ4_CORRUPT;               // a sequence starts with a token
      const uint32_t token = byte_at(sp++);
      uint32_t ll = token >> 4;
      if (ll == 15 && !extend(&sp, &ll)) return AH_LZ4_CORRUPT;
      if (ll > slen - sp || ll > dlen - op) return AH_LZ4_CORRUPT;   // literals past the source end / past the output
      literals(sp, op, ll);
      sp += ll; op += ll;
      if (sp == slen) break;                                 // the last sequence has no match
      if (slen - sp < 2) return AH_LZ4_CORRUPT;
      ensure(sp, 2);
      const uint32_t at = sp + mis - wv;
      const uint32_t offset = par.uni((uint32_t)win[at] | ((uint32_t)win[at + 1] << 8));
      sp += 2;
      if (offset == 0 || offset > op) return AH_LZ4_CORRUPT;         // before the block's first byte
      uint32_t ml = token & 15;
      if (ml == 15 && !extend(&sp, &ml)) return AH_LZ4_CORRUPT;
      ml += 4;
      if (ml > dlen - op) return AH_LZ4_CORRUPT;
      uint8_t* im = image;
      par.lanes([=](int lane, int nlanes) { ah_lz4_copy_match(im, op, offset, ml, lane, nlanes); });
      op += ml;
    }
    return op == dlen ? AH_LZ4_OK : AH_LZ4_WRONG_SIZE;
  }
};

// One block: src[0, slen) → dst[0, dlen) through `image` and `win`.  dst is written only when the status is AH_LZ4_OK.
template <class Par>
AH_LZ4_HD int ah_lz4_decode_block(Par& par, const uint8_t* src, uint32_t slen, bool stored, uint8_t* dst, uint32_t dlen, uint8_t* image, uint8_t* win) {
  ah_lz4_decoder<Par> d{par, src, slen, image, dlen, win, 0, 0};
  const int st = d.run(stored);
  if (st == AH_LZ4_OK && dlen > 0) par.lanes([=](int lane, int nlanes) { ah_lz4_flush(dst, image, dlen, lane, nlanes); });
  return st;
}
