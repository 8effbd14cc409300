// like_program_harness.cc — the LIKE compiler of arrow_go_amd/host/like_program.h as a stand-alone host program, for
// tests/test_string_match_model_host.py to build with -fsanitize=address,undefined: one pattern per input line as hex ("-" for the
// empty pattern), one program per output line as hex.  The pattern is copied into a heap block of exactly its size, so a read
// past either end is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../arrow_go_amd/host/like_program.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line == "-") line.clear();
    const size_t n = line.size() / 2;
    uint8_t* pattern = (uint8_t*)malloc(n ? n : 1);
    for (size_t i = 0; i < n; i++) pattern[i] = (uint8_t)strtoul(line.substr(2 * i, 2).c_str(), nullptr, 16);
    const std::vector<uint8_t> program = arrowhip::like::Compile(pattern, n);
    free(pattern);
    for (uint8_t b : program) printf("%02x", b);
    printf("\n");
  }
  return 0;
}
