// strconv_harness.cc — csrc/ah_strconv.h compiled for the host: each routine over `count` rows of a byte column with 64-bit
// offsets (tests/test_strconv_host.py compares them with Python).  Every row is copied into a buffer of exactly its length, so a
// read outside the row is a read outside an allocation.
#include "../arrow_go_amd/csrc/ah_strconv.h"

#include <cstdlib>
#include <cstring>

namespace {

struct HostRow {
  const uint8_t* p;
  int64_t len;
  unsigned long long word(int64_t i) const {
    unsigned long long w = 0;
    memcpy(&w, p + i, (size_t)(len - i >= 8 ? 8 : len - i));
    return w;
  }
};

struct Copy {  // the row alone in an allocation of its own size
  uint8_t* q;
  HostRow row;
  Copy(const uint8_t* data, const long long* offsets, long i) {
    const int64_t len = offsets[i + 1] - offsets[i];
    q = (uint8_t*)malloc(len ? (size_t)len : 1);
    memcpy(q, data + offsets[i], (size_t)len);
    row = HostRow{q, len};
  }
  ~Copy() { free(q); }
};

}  // namespace

extern "C" {

void sh_parse_int(const uint8_t* data, const long long* offsets, long count, int bits, int is_signed, unsigned long long* values,
                  unsigned char* kinds) {
  for (long i = 0; i < count; i++) {
    Copy c(data, offsets, i);
    kinds[i] = (unsigned char)sc_parse_int(c.row, bits, is_signed != 0, &values[i]);
  }
}

void sh_parse_bool(const uint8_t* data, const long long* offsets, long count, unsigned char* values, unsigned char* kinds) {
  for (long i = 0; i < count; i++) {
    Copy c(data, offsets, i);
    int v = 0;
    kinds[i] = (unsigned char)sc_parse_bool(c.row, &v);
    values[i] = (unsigned char)v;
  }
}

// 20 bytes per row in `chars`, '\0' behind the last character
void sh_format_int(const unsigned long long* values, long count, int is_signed, int* lens, uint8_t* chars) {
  for (long i = 0; i < count; i++) {
    lens[i] = sc_format_len(values[i], is_signed != 0);
    memset(chars + i * 20, 0, 20);
    sc_format_write(values[i], is_signed != 0, chars + i * 20, lens[i]);
  }
}

void sh_format_bool(int v, int* len, uint8_t* chars) {
  *len = sc_format_bool_len(v);
  sc_format_bool_write(v, chars);
}

// piece = 0: utf8.Valid of the whole row; else the row in pieces of `piece` bytes, valid when every piece is
void sh_utf8_valid(const uint8_t* data, const long long* offsets, long count, long piece, unsigned char* ok) {
  for (long i = 0; i < count; i++) {
    Copy c(data, offsets, i);
    bool good = true;
    if (piece == 0) good = sc_utf8_valid(c.row);
    else
      for (int64_t from = 0; from < c.row.len; from += piece) good = sc_utf8_valid_range(c.row, from, from + piece) && good;
    ok[i] = good ? 1 : 0;
  }
}

}  // extern "C"
