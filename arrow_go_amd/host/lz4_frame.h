// LZ4 frame → a plan of independent blocks for the device decoder (ah_lz4_decompress_blocks), or "does not qualify".
//
// lz4_Frame_format.md: magic 0x184D2204 | FLG | BD | [content size, 8] | [DictID, 4] | HC | { block size (u32; bit 31: stored) |
// block }… | EndMark (u32 0) | [content checksum, 4].  FLG: bits 7-6 version (01), 5 block independence, 4 block checksum,
// 3 content size, 2 content checksum, 1 reserved, 0 DictID.  BD: bits 6-4 block maximum (4: 64 KiB), the rest reserved.
// HC: second byte of xxh32 of the descriptor (FLG … before HC), seed 0.
//
// The reference's writer (arrow/ipc/compression.go:66-72) asks pierrec/lz4 for 64 KiB blocks without a content checksum; whether a
// frame can be decoded block by block is decided here from its own FLG byte, never assumed.  The format stores no output size per
// block: the plan takes every block but the last for exactly 64 KiB and the decoder reports a block that is not (status 2), after
// which the caller inflates the frame the way it always did.  A frame that does not qualify is not an error here.
//
// Plain C++ without the library's types: tests/lz4_harness.cc includes this file.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace arrowhip {
namespace lz4 {

constexpr int64_t kBlockMax = 65536;

inline uint32_t Xxh32(const uint8_t* p, size_t n, uint32_t seed) {
  constexpr uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
  auto rotl = [](uint32_t x, int r) { return (x << r) | (x >> (32 - r)); };
  auto rd32 = [](const uint8_t* q) { return (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24; };
  const uint8_t* end = p + n;
  uint32_t h;
  if (n >= 16) {
    uint32_t v1 = seed + P1 + P2, v2 = seed + P2, v3 = seed, v4 = seed - P1;
    for (; p + 16 <= end; p += 16) {
      v1 = rotl(v1 + rd32(p) * P2, 13) * P1;
      v2 = rotl(v2 + rd32(p + 4) * P2, 13) * P1;
      v3 = rotl(v3 + rd32(p + 8) * P2, 13) * P1;
      v4 = rotl(v4 + rd32(p + 12) * P2, 13) * P1;
    }
    h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
  } else {
    h = seed + P5;
  }
  h += (uint32_t)n;
  for (; p + 4 <= end; p += 4) h = rotl(h + rd32(p) * P3, 17) * P4;
  for (; p < end; p++) h = rotl(h + *p * P5, 11) * P1;
  h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
  return h;
}

struct Block {
  int64_t src_off, src_len;   // inside the frame
  int64_t dst_off, dst_len;   // inside the frame's `ulen` output bytes
  bool stored;
};

// true: `frame` can be decoded block by block into `ulen` bytes, *out holds its blocks (none for ulen == 0)
inline bool PlanFrame(const uint8_t* frame, int64_t n, int64_t ulen, std::vector<Block>* out) {
  out->clear();
  auto rd32 = [&](int64_t at) { return (uint32_t)frame[at] | (uint32_t)frame[at + 1] << 8 | (uint32_t)frame[at + 2] << 16 | (uint32_t)frame[at + 3] << 24; };
  if (ulen < 0 || n < 4 + 3 + 4) return false;   // magic, the shortest descriptor, EndMark
  if (rd32(0) != 0x184D2204u) return false;
  const uint8_t flg = frame[4], bd = frame[5];
  if ((flg >> 6) != 1) return false;                  // version
  if (!(flg & 0x20)) return false;                    // blocks refer to their predecessors
  if (flg & 0x10) return false;                       // block checksums
  if (flg & 0x04) return false;                       // content checksum
  if (flg & 0x02) return false;                       // reserved
  if (flg & 0x01) return false;                       // DictID
  if (bd & 0x8F) return false;                        // reserved
  if (((bd >> 4) & 7) != 4) return false;             // block maximum other than 64 KiB
  int64_t at = 6;
  if (flg & 0x08) {
    if (n < at + 8 + 1 + 4) return false;
    uint64_t csize;
    std::memcpy(&csize, frame + at, 8);
    if (csize != (uint64_t)ulen) return false;
    at += 8;
  }
  if (((Xxh32(frame + 4, (size_t)(at - 4), 0) >> 8) & 0xFF) != frame[at]) return false;
  at += 1;
  const int64_t want = (ulen + kBlockMax - 1) / kBlockMax;
  int64_t produced = 0;
  for (;;) {
    if (n - at < 4) return false;
    const uint32_t word = rd32(at);
    at += 4;
    if (word == 0) break;                             // EndMark
    const int64_t size = (int64_t)(word & 0x7FFFFFFFu);
    if (size > kBlockMax || size > n - at) return false;
    if ((int64_t)out->size() >= want) return false;   // more blocks than ulen bytes can fill
    const int64_t left = ulen - produced;
    const int64_t dlen = left < kBlockMax ? left : kBlockMax;
    out->push_back({at, size, produced, dlen, (word >> 31) != 0});
    produced += dlen;
    at += size;
  }
  if (at != n) return false;                          // bytes behind the EndMark
  return (int64_t)out->size() == want;
}

}  // namespace lz4
}  // namespace arrowhip
