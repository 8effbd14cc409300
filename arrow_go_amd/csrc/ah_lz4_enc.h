// ah_lz4_enc.h — one LZ4 block compressed by a group of cooperating lanes, the mirror image of ah_lz4.h.  Compiled
// for the device (ah_lz4_enc.hip: the 64 lanes of a wavefront) and for the host (tests/lz4_enc_harness.cc: lanes 0 … 63 in a loop) from
// the same text; only `Par` differs.  Beside the decoder's three it needs one more way for the lanes to agree:
//
//   Par::lanes(f)   every lane runs f(lane, nlanes); when it returns, what the lanes wrote is visible to all of them
//   Par::sync()     what the lanes read before it is read before anything after it is written
//   Par::uni(x)     x, which is the same in every lane, as a value the compiler may keep in a scalar register
//   Par::first(f)   the lowest lane for which f(lane, nlanes) is true, nlanes if there is none (a ballot); f only reads
//
// The scheme, one step over the 64 positions p … p + 63 of the block image:
//   probe    lane i hashes the 4 bytes at p + i, reads the table's 16-bit position for that hash and keeps it as its candidate if
//            it lies below p + i and its 4 bytes are the same.  (A slot never written holds 0: position 0 is a candidate like any
//            other, so the table needs no "empty" mark.)  All probes of a step see the table as the previous step left it.
//   match    first() picks the lowest lane with a candidate at or behind the end of the previous match; the lanes extend it
//            together, 64 bytes per first(), up to 5 bytes before the block's end; the sequence {literals since the last match,
//            offset, length} is written; the search goes on among the step's remaining lanes behind the match.
//   publish  every lane of the step stores its position in its hash's slot.  Where several lanes of one step share a slot the
//            HIGHEST position wins, by rule: after the store every lane reads the slot back and stores again while it holds a
//            lower position than its own — the slot's value only grows, so this ends after at most nlanes rounds (one, where the
//            lanes run in a loop), and what it ends with does not depend on which lane the hardware let win a round.
//   The next step starts at p + 64, or behind the last match if that lies further on.
// Nothing a lane reads inside one lanes() call is written by another lane in the same call, so lanes that run one after the other
// and lanes that run together compute the same bytes: the output is a function of the input alone.
//
// The format rules (lz4_Block_format.md) hold by construction: a match starts at a position q with q + 12 ≤ n and ends at or before
// n − 5, so the last 5 bytes are literals and a block under 13 bytes has no match; a candidate lies below its position, so
// 1 ≤ offset ≤ q ≤ 65 523; a length nibble of 15 is followed by 255-chained bytes.  The output leaves through a 4 KiB window the
// lanes drain with 16-byte stores; a sequence is written only if the block stays SMALLER than its input with it — otherwise the
// block is "stored": the slot receives the input bytes themselves.  Every byte written lies in dst[0, n).  No loop waits for
// anything: each one advances a position or a byte count of this block.
#pragma once
#include "ah_lz4.h"

constexpr uint32_t kLz4EncHashBits = 12;
constexpr uint32_t kLz4EncTable = 1u << kLz4EncHashBits;   // 16-bit positions: 8 KiB
constexpr uint32_t kLz4EncOutWindow = 4096;                // bytes (a multiple of 16)
constexpr uint32_t kLz4EncMaxLanes = 64;
constexpr uint32_t kLz4EncNoCand = 1u << 16;               // lane state: bits 0-15 candidate, bit 16 none, bits 17-28 hash, bit 31 active
constexpr uint32_t kLz4EncActive = 1u << 31;
constexpr uint32_t kLz4MinMatch = 4, kLz4LastLiterals = 5, kLz4MatchSafe = 12;

AH_LZ4_HD uint32_t ah_lz4_read32(const uint8_t* p) {   // byte by byte: the position has any alignment
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
AH_LZ4_HD void ah_lz4_put32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}
AH_LZ4_HD uint32_t ah_lz4_hash(uint32_t v) { return (v * 2654435761u) >> (32 - kLz4EncHashBits); }

// the block's n bytes → image[0, n): 16-byte loads from aligned addresses, the two ends byte by byte inside the block only
AH_LZ4_HD void ah_lz4_stage(uint8_t* image, const uint8_t* src, uint32_t n, uint32_t mis, int lane, int nlanes) {
  const uint32_t nslots = (n + mis + 15) / 16;
  for (uint32_t j = (uint32_t)lane; j < nslots; j += (uint32_t)nlanes) {
    const int64_t b0 = 16 * (int64_t)j - (int64_t)mis;   // block position of the slot's first byte
    if (b0 >= 0 && b0 + 16 <= (int64_t)n) {
      if (mis == 0) {
        ah_lz4_move16(image + b0, src + b0);
      } else {
        struct alignas(16) { uint32_t a, b, c, d; } t;   // (four words, not an array: they stay in registers)
        ah_lz4_move16(reinterpret_cast<uint8_t*>(&t), src + b0);
        ah_lz4_put32(image + b0, t.a); ah_lz4_put32(image + b0 + 4, t.b); ah_lz4_put32(image + b0 + 8, t.c); ah_lz4_put32(image + b0 + 12, t.d);
      }
    } else {
      for (int k = 0; k < 16; k++) {
        const int64_t b = b0 + k;
        if (b >= 0 && b < (int64_t)n) image[b] = src[b];
      }
    }
  }
}

// one sequence as a function index → byte: token, literal length bytes, literals, offset, match length bytes
struct ah_lz4_seq {
  uint32_t lit_at, ll, lle;   // literals image[lit_at, lit_at + ll); lle extension bytes
  uint32_t offset, ml, mle;   // ml = match length − 4; offset 0: the block's last sequence, which has no match
  uint32_t size;
};
AH_LZ4_HD uint32_t ah_lz4_ext_count(uint32_t len) { return len < 15 ? 0 : (len - 15) / 255 + 1; }
AH_LZ4_HD uint32_t ah_lz4_ext_byte(uint32_t len, uint32_t count, uint32_t j) { return j + 1 < count ? 255u : (len - 15) % 255; }
AH_LZ4_HD ah_lz4_seq ah_lz4_make_seq(uint32_t lit_at, uint32_t ll, uint32_t offset, uint32_t match_len) {
  ah_lz4_seq s;
  s.lit_at = lit_at; s.ll = ll; s.lle = ah_lz4_ext_count(ll);
  s.offset = offset; s.ml = offset ? match_len - kLz4MinMatch : 0; s.mle = offset ? ah_lz4_ext_count(s.ml) : 0;
  s.size = 1 + s.lle + ll + (offset ? 2 + s.mle : 0);
  return s;
}
AH_LZ4_HD uint8_t ah_lz4_seq_byte(const ah_lz4_seq& s, const uint8_t* image, uint32_t i) {
  if (i == 0) return (uint8_t)(((s.ll < 15 ? s.ll : 15) << 4) | (s.ml < 15 ? s.ml : 15));
  i -= 1;
  if (i < s.lle) return (uint8_t)ah_lz4_ext_byte(s.ll, s.lle, i);
  i -= s.lle;
  if (i < s.ll) return image[s.lit_at + i];
  i -= s.ll;
  if (i == 0) return (uint8_t)(s.offset & 255);
  if (i == 1) return (uint8_t)(s.offset >> 8);
  return (uint8_t)ah_lz4_ext_byte(s.ml, s.mle, i - 2);
}

// window bytes [max(wv, lo), hi) → dst: positions are "virtual" (output position + the slot's misalignment), so a virtual multiple
// of 16 is a 16-byte aligned address; a 16-byte line that lies inside [lo, hi) is one vector store, the lines at the ends go byte by byte
AH_LZ4_HD void ah_lz4_drain(uint8_t* dst, const uint8_t* win, uint32_t mis, uint32_t wv, uint32_t lo, uint32_t hi, int lane, int nlanes) {
  for (uint32_t j = (uint32_t)lane; j < kLz4EncOutWindow / 16; j += (uint32_t)nlanes) {
    const uint32_t v0 = wv + 16 * j;
    if (v0 >= hi) break;
    if (v0 >= lo && v0 + 16 <= hi) {
      ah_lz4_move16(dst + (v0 - mis), win + 16 * j);
    } else {
      for (uint32_t k = 0; k < 16; k++)
        if (v0 + k >= lo && v0 + k < hi) dst[v0 + k - mis] = win[16 * j + k];
    }
  }
}

template <class Par>
struct ah_lz4_encoder {
  Par& par;
  uint8_t* image;     // ≥ n bytes, 16-byte aligned: the block
  uint32_t n;
  uint16_t* table;    // kLz4EncTable positions, 16-byte aligned
  uint32_t* state;    // kLz4EncMaxLanes words: what a lane found in the probe of this step
  uint8_t* win;       // kLz4EncOutWindow bytes, 16-byte aligned
  uint8_t* dst;       // the slot: n bytes
  uint32_t mis, wv, on;   // slot misalignment; the window's first virtual position; bytes produced
  bool fits;              // on < n so far; once false nothing more is written and `on` only counts what the block would take

  // the sequence's bytes behind the on produced so far, if the block stays smaller than n with them
  AH_LZ4_HD void emit(const ah_lz4_seq& s) {
    if (!fits || s.size >= n - on) {
      fits = false;
      on += s.size;
      return;
    }
    uint32_t done = 0;
    while (done < s.size) {
      const uint32_t at = on + mis - wv, room = kLz4EncOutWindow - at;
      if (room == 0) {
        uint8_t* d = dst;
        const uint8_t* w = win;
        const uint32_t m = mis, base = wv;
        par.lanes([=](int lane, int nlanes) { ah_lz4_drain(d, w, m, base, m, base + kLz4EncOutWindow, lane, nlanes); });
        wv += kLz4EncOutWindow;
        continue;
      }
      const uint32_t m = s.size - done < room ? s.size - done : room;
      uint8_t* to = win + at;
      const uint8_t* im = image;
      par.lanes([=](int lane, int nlanes) {
        for (uint32_t i = (uint32_t)lane; i < m; i += (uint32_t)nlanes) to[i] = ah_lz4_seq_byte(s, im, done + i);
      });
      done += m; on += m;
    }
  }

  // → bytes written to dst[0, …): the compressed block, or the n input bytes where that would not be smaller ("stored").
  // *lz4_size: what the block takes compressed, written or not — stored ⇔ *lz4_size ≥ n
  AH_LZ4_HD uint32_t run(const uint8_t* src, uint32_t* lz4_size) {
    *lz4_size = 1;   // (n == 0: the token of an empty last sequence)
    if (n == 0 || n > kLz4MaxBlock) return 0;
    {
      uint8_t* im = image;
      uint16_t* tb = table;
      const uint32_t len = n, smis = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15);
      par.sync();
      par.lanes([=](int lane, int nlanes) {
        ah_lz4_stage(im, src, len, smis, lane, nlanes);
        for (uint32_t j = (uint32_t)lane; j < kLz4EncTable; j += (uint32_t)nlanes) tb[j] = 0;
      });
    }
    mis = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15);
    wv = 0; on = 0; fits = true;
    uint32_t anchor = 0, p = 0;
    while (p + kLz4MatchSafe <= n) {
      const uint8_t* im = image;
      uint16_t* tb = table;
      uint32_t* st = state;
      const uint32_t len = n, base = p;
      par.lanes([=](int lane, int) {   // probe
        const uint32_t q = base + (uint32_t)lane;
        uint32_t w = 0;
        if (q + kLz4MatchSafe <= len) {
          const uint32_t v = ah_lz4_read32(im + q), h = ah_lz4_hash(v), c = tb[h];
          w = kLz4EncActive | (h << 17) | ((c < q && ah_lz4_read32(im + c) == v) ? c : kLz4EncNoCand);
        }
        st[lane] = w;
      });
      uint32_t lo = 0;   // (anchor ≤ p at the start of a step)
      for (;;) {
        const uint32_t from = lo;
        const uint32_t k = par.uni(par.first([=](int lane, int) {
          return (uint32_t)lane >= from && (st[lane] & (kLz4EncActive | kLz4EncNoCand)) == kLz4EncActive; }));
        if (k >= kLz4EncMaxLanes) break;
        const uint32_t q = p + k, c = par.uni(st[k] & 0xFFFFu), maxlen = n - kLz4LastLiterals - q;
        uint32_t ml = kLz4MinMatch;
        for (;;) {   // 64 bytes per round; ml never passes maxlen
          const uint32_t have = ml;
          const uint32_t j = par.uni(par.first([=](int lane, int) {
            const uint32_t t = have + (uint32_t)lane;
            return t >= maxlen || im[c + t] != im[q + t]; }));
          ml += j;
          if (j < kLz4EncMaxLanes) break;
        }
        emit(ah_lz4_make_seq(anchor, q - anchor, q - c, ml));
        anchor = q + ml;
        if (anchor >= p + kLz4EncMaxLanes) break;
        lo = anchor - p;
      }
      par.sync();
      par.lanes([=](int lane, int) {   // publish
        const uint32_t w = st[lane];
        if (w & kLz4EncActive) tb[(w >> 17) & (kLz4EncTable - 1)] = (uint16_t)(base + (uint32_t)lane);
      });
      for (uint32_t round = 0; round < kLz4EncMaxLanes; round++) {   // the highest position of a shared slot wins
        const uint32_t low = par.uni(par.first([=](int lane, int) {
          const uint32_t w = st[lane];
          return (w & kLz4EncActive) != 0 && tb[(w >> 17) & (kLz4EncTable - 1)] < base + (uint32_t)lane; }));
        if (low >= kLz4EncMaxLanes) break;
        par.sync();
        par.lanes([=](int lane, int) {
          const uint32_t w = st[lane], q = base + (uint32_t)lane;
          if ((w & kLz4EncActive) && tb[(w >> 17) & (kLz4EncTable - 1)] < q) tb[(w >> 17) & (kLz4EncTable - 1)] = (uint16_t)q;
        });
      }
      const uint32_t next = p + kLz4EncMaxLanes;
      p = anchor > next ? anchor : next;
    }
    emit(ah_lz4_make_seq(anchor, n - anchor, 0, 0));
    const uint32_t len = n, produced = on, m = mis, base = wv;
    const bool stored = !fits;
    *lz4_size = produced;
    uint8_t* d = dst;
    const uint8_t* im = image;
    const uint8_t* w = win;
    par.lanes([=](int lane, int nlanes) {
      if (stored) ah_lz4_flush(d, im, len, lane, nlanes);
      else ah_lz4_drain(d, w, m, base, m, produced + m, lane, nlanes);
    });
    return stored ? len : produced;
  }
};

// One block: src[0, n) → dst[0, returned size); the slot dst has n bytes.  *lz4_size ≥ n: the block did not shrink and dst holds
// src's bytes ("stored"); else *lz4_size is the returned size.
template <class Par>
AH_LZ4_HD uint32_t ah_lz4_encode_block(Par& par, const uint8_t* src, uint32_t n, uint8_t* dst, uint8_t* image, uint16_t* table, uint32_t* state,
                                       uint8_t* win, uint32_t* lz4_size) {
  ah_lz4_encoder<Par> e{par, image, n, table, state, win, dst, 0, 0, 0, true};
  return e.run(src, lz4_size);
}
