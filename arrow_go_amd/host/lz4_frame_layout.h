// Block sizes → where every part of one IPC body buffer lands (the writer's side of lz4_frame.h).
//
// A compressed buffer of an IPC body (arrow/ipc/compression.go, format/Message.fbs BodyCompression, method BUFFER) is
//   int64 LE uncompressed length | LZ4 frame            … or …        int64 LE −1 | the raw bytes
// and the frame this writer makes is the one the reader's device path accepts: magic 0x184D2204 | FLG 0x60 (version 01, independent
// blocks) | BD 0x40 (64 KiB) | HC | { u32 LE block size, bit 31 = stored | block }… | u32 0, no content size and no checksums.
// Every buffer starts on a multiple of 8 of the body; the bytes up to the next multiple of 8 behind it are zero.
//
// Pure arithmetic: sizes in, offsets out.  Plain C++ without the library's types: tests/lz4_enc_harness.cc includes this file.
#pragma once
#include <cstdint>
#include <vector>

#include "lz4_frame.h"

namespace arrowhip {
namespace lz4 {

constexpr int64_t kFramePrefix = 8;   // the uncompressed length in front of a compressed buffer
constexpr int64_t kFrameHeader = 7;   // magic, FLG, BD, HC
constexpr uint8_t kFrameFlg = 0x60, kFrameBd = 0x40;

// the 7 bytes every frame of this writer starts with
inline void FrameHeader(uint8_t out[7]) {
  out[0] = 0x04; out[1] = 0x22; out[2] = 0x4D; out[3] = 0x18;
  out[4] = kFrameFlg; out[5] = kFrameBd;
  out[6] = (uint8_t)((Xxh32(out + 4, 2, 0) >> 8) & 0xFF);
}

// prefix + frame of blocks with these sizes
inline int64_t FramedBytes(const std::vector<int64_t>& sizes) {
  int64_t n = kFramePrefix + kFrameHeader + 4;
  for (int64_t s : sizes) n += 4 + s;
  return n;
}
inline int64_t Pad8(int64_t n) { return (n + 7) & ~(int64_t)7; }

struct FrameLayout {
  int64_t prefix_at = 0, header_at = 0;   // the 8-byte length; the 7-byte frame header
  std::vector<int64_t> block_at;          // the 4-byte size word of block i; its bytes follow at block_at[i] + 4
  int64_t end_mark_at = 0, end = 0;       // the 4-byte EndMark; the first byte behind it
  int64_t padded_end = 0;                 // end rounded up to 8: where the next buffer starts; [end, padded_end) is zero
};
// the buffer starts at body offset `at` (a multiple of 8)
inline FrameLayout LayoutFrame(int64_t at, const std::vector<int64_t>& sizes) {
  FrameLayout f;
  f.prefix_at = at;
  f.header_at = at + kFramePrefix;
  int64_t p = f.header_at + kFrameHeader;
  for (int64_t s : sizes) {
    f.block_at.push_back(p);
    p += 4 + s;
  }
  f.end_mark_at = p;
  f.end = p + 4;
  f.padded_end = Pad8(f.end);
  return f;
}

}  // namespace lz4
}  // namespace arrowhip
