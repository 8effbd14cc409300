// The LZ4 block decoder (csrc/ah_lz4.h) and the frame planner (host/lz4_frame.h) as a stand-alone host program, for
// tests/test_lz4_host.py: built with -fsanitize=address,undefined, fed hex vectors on stdin, one answer per line on stdout.
//
//   B <stored 0|1> <dst_len> <misalignment 0…15> <hex of the block | ->    →  <status> [<hex of the dst_len output bytes> | -]
//   P <ulen> <hex of the frame>                                              →  0   |   1 <n> {<src_off> <src_len> <dst_off> <dst_len> <stored>}…
//
// The decoder runs exactly as on the device, with the 64 lanes of a wavefront one after the other in a loop.  Every buffer is a heap
// allocation of exactly the size the decoder is told (source, output, 64 KiB image, window), so a read or write outside one is a
// sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../arrow_go_amd/csrc/ah_lz4.h"
#include "../arrow_go_amd/host/lz4_frame.h"

namespace {

struct LoopPar {
  template <class F>
  void lanes(F&& f) {
    for (int lane = 0; lane < 64; lane++) f(lane, 64);
  }
  void sync() {}
  uint32_t uni(uint32_t x) { return x; }
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
  uint8_t* image = aligned(kLz4MaxBlock);
  uint8_t* win = aligned(kLz4Window);
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind == "B") {
      int stored, mis;
      long long dlen;
      std::string h;
      in >> stored >> dlen >> mis >> h;
      const std::vector<uint8_t> bytes = unhex(h);
      if (dlen < 0 || dlen > (long long)kLz4MaxBlock || mis < 0 || mis > 15) { std::puts("bad vector"); return 2; }
      uint8_t* sbuf = aligned((size_t)mis + bytes.size());   // the block ends where the allocation ends
      if (!bytes.empty()) std::memcpy(sbuf + mis, bytes.data(), bytes.size());
      uint8_t* dst = aligned((size_t)dlen);
      std::memset(image, 0xEE, kLz4MaxBlock);
      std::memset(win, 0xEE, kLz4Window);
      LoopPar par;
      const int st = ah_lz4_decode_block(par, sbuf + mis, (uint32_t)bytes.size(), stored != 0, dst, (uint32_t)dlen, image, win);
      std::printf("%d %s\n", st, st == 0 ? hex(dst, (size_t)dlen).c_str() : "-");
      free(sbuf);
      free(dst);
    } else if (kind == "P") {
      long long ulen;
      std::string h;
      in >> ulen >> h;
      const std::vector<uint8_t> bytes = unhex(h);
      uint8_t* f = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);
      if (!bytes.empty()) std::memcpy(f, bytes.data(), bytes.size());
      std::vector<arrowhip::lz4::Block> blocks;
      const bool ok = arrowhip::lz4::PlanFrame(f, (int64_t)bytes.size(), ulen, &blocks);
      if (!ok) {
        std::puts("0");
      } else {
        std::printf("1 %zu", blocks.size());
        for (const auto& b : blocks) std::printf(" %lld %lld %lld %lld %d", (long long)b.src_off, (long long)b.src_len, (long long)b.dst_off, (long long)b.dst_len, b.stored ? 1 : 0);
        std::puts("");
      }
      free(f);
    } else if (!kind.empty()) {
      std::puts("bad vector");
      return 2;
    }
  }
  free(image);
  free(win);
  return 0;
}
