// The LZ4 block compressor (csrc/ah_lz4_enc.h) and the frame layout of the IPC writer (host/lz4_frame_layout.h) as a stand-alone
// host program, for tests/test_lz4_enc_host.py and tests/test_ipc_writer.py: built with -fsanitize=address,undefined, fed hex
// vectors on stdin, one answer per line on stdout.
//
//   C <src misalignment 0…15> <dst misalignment 0…15> <hex of the block | ->   →  <stored 0|1> <size as an LZ4 block> <hex of the bytes written | ->
//   L <at> <block size>…                                                        →  <prefix_at> <header_at> <hex of the 7 header bytes> <end_mark_at> <end> <padded_end> <block_at>…
//
// The compressor runs exactly as on the device, with the 64 lanes of a wavefront one after the other in a loop.  Every buffer is a
// heap allocation of exactly the size the compressor is told (source, slot, image, table, lane state, window), so a read or write
// outside one is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../arrow_go_amd/csrc/ah_lz4_enc.h"
#include "../arrow_go_amd/host/lz4_frame_layout.h"

namespace {

struct LoopPar {
  template <class F>
  void lanes(F&& f) {
    for (int lane = 0; lane < 64; lane++) f(lane, 64);
  }
  void sync() {}
  uint32_t uni(uint32_t x) { return x; }
  template <class F>
  uint32_t first(F&& f) {
    for (int lane = 0; lane < 64; lane++)
      if (f(lane, 64)) return (uint32_t)lane;
    return 64;
  }
};

std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> out;
  if (h == "-") return out;
  auto nib = [](char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; };
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)(nib(h[i]) << 4 | nib(h[i + 1])));
  return out;
}
std::string hex(const uint8_t* p, size_t n) {
  if (n == 0) return "-";
  static const char* d = "0123456789abcdef";
  std::string s(2 * n, '0');
  for (size_t i = 0; i < n; i++) { s[2 * i] = d[p[i] >> 4]; s[2 * i + 1] = d[p[i] & 15]; }
  return s;
}
uint8_t* aligned(size_t n) {
  void* p = nullptr;
  if (posix_memalign(&p, 16, n ? n : 1) != 0) abort();
  return (uint8_t*)p;
}

}  // namespace

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind == "C") {
      int smis, dmis;
      std::string h;
      in >> smis >> dmis >> h;
      const std::vector<uint8_t> bytes = unhex(h);
      const size_t n = bytes.size();
      if (n > kLz4MaxBlock || smis < 0 || smis > 15 || dmis < 0 || dmis > 15) { std::puts("bad vector"); return 2; }
      uint8_t* sbuf = aligned((size_t)smis + n);   // the block ends where the allocation ends
      if (n) std::memcpy(sbuf + smis, bytes.data(), n);
      uint8_t* dbuf = aligned((size_t)dmis + n);   // … and so does its slot
      uint8_t* image = aligned(n);
      uint16_t* table = (uint16_t*)aligned(kLz4EncTable * sizeof(uint16_t));
      uint32_t* state = (uint32_t*)aligned(kLz4EncMaxLanes * sizeof(uint32_t));
      uint8_t* win = aligned(kLz4EncOutWindow);
      std::memset(dbuf, 0xEE, (size_t)dmis + n);
      std::memset(image, 0xEE, n);
      std::memset(table, 0xEE, kLz4EncTable * sizeof(uint16_t));
      std::memset(state, 0xEE, kLz4EncMaxLanes * sizeof(uint32_t));
      std::memset(win, 0xEE, kLz4EncOutWindow);
      LoopPar par;
      uint32_t lz4_size = 0;
      const uint32_t size = ah_lz4_encode_block(par, sbuf + smis, (uint32_t)n, dbuf + dmis, image, table, state, win, &lz4_size);
      const bool stored = lz4_size >= n;
      bool guard = true;
      for (int i = 0; i < dmis; i++) guard = guard && dbuf[i] == 0xEE;
      if (size > n || !guard) { std::puts("wrote outside the slot"); return 3; }
      std::printf("%d %u %s\n", stored ? 1 : 0, lz4_size, hex(dbuf + dmis, size).c_str());
      free(sbuf); free(dbuf); free(image); free(table); free(state); free(win);
    } else if (kind == "L") {
      long long at, s;
      in >> at;
      std::vector<int64_t> sizes;
      while (in >> s) sizes.push_back(s);
      const arrowhip::lz4::FrameLayout f = arrowhip::lz4::LayoutFrame(at, sizes);
      uint8_t head[7];
      arrowhip::lz4::FrameHeader(head);
      std::printf("%lld %lld %s %lld %lld %lld", (long long)f.prefix_at, (long long)f.header_at, hex(head, 7).c_str(), (long long)f.end_mark_at,
                  (long long)f.end, (long long)f.padded_end);
      for (int64_t b : f.block_at) std::printf(" %lld", (long long)b);
      std::puts("");
      if (f.end - at != arrowhip::lz4::FramedBytes(sizes)) { std::puts("FramedBytes disagrees"); return 3; }
    } else if (!kind.empty()) {
      std::puts("bad vector");
      return 2;
    }
  }
  return 0;
}
