// ah_strconv.h — the conversion rules of the string casts (ah_cast_string.hip): Go's strconv.ParseInt / ParseUint with base 0,
// strconv.ParseBool, strconv.FormatInt / FormatUint in base 10, and utf8.Valid.  What getParseStringExec
// (arrow/compute/internal/kernels/numeric_cast.go:742-781), the ParseBool kernels (boolean_cast.go:77-95), the numeric → string
// formatters (string_casts.go) and validateUTF8Sequence (string_casts.go:39-48) call, row by row.
//
// Compiles for the device and for the host (tests/strconv_harness.cc checks every routine against Python on the CPU).  No global
// state.  A row is seen through a reader R with two members: `len`, its length in bytes, and `word(i)`, the 8 bytes at i (0 ≤ i < len,
// any alignment) as a little-endian number, ZERO where the row has ended — a reader never touches a byte outside the row.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AH_SC_FN __device__ __forceinline__
#else
#define AH_SC_FN static inline
#endif

enum { kScOk = 0, kScSyntax = 1, kScRange = 2 };  // strconv.ErrSyntax / strconv.ErrRange

// strconv.ParseInt(s, 0, bits) (is_signed) / strconv.ParseUint(s, 0, bits): the value in *out (a signed one sign-extended to
// 64 bits), or the FIRST error in scan order — ParseUint returns a range error at the digit that overflows, before it has seen
// what follows, and checks the underscores (underscoreOK) only after the last byte.
template <class R>
AH_SC_FN int sc_parse_int(const R& r, int bits, bool is_signed, unsigned long long* out) {
  *out = 0;
  const int64_t len = r.len;
  if (len == 0) return kScSyntax;
  const unsigned long long w0 = r.word(0);
  int64_t i = 0;
  bool neg = false;
  if (is_signed) {  // ParseUint takes no sign: its '+' / '-' is a bad byte below
    const unsigned c = (unsigned)(w0 & 0xFF);
    if (c == '+' || c == '-') {
      neg = c == '-';
      i = 1;
      if (len == 1) return kScSyntax;
    }
  }
  // base 0: the prefix decides; at least one digit must follow 0x / 0b / 0o, so a two-byte "0x" is octal "0" + the bad byte 'x'
  unsigned base = 10;
  char saw = '^';  // underscoreOK's state: '0' a digit or the base prefix, '_' an underscore
  const unsigned a = (unsigned)(w0 >> (8 * i)) & 0xFF, b = ((unsigned)(w0 >> (8 * (i + 1))) & 0xFF) | 0x20;
  if (a == '0') {
    saw = '0';
    if (len - i >= 3 && (b == 'b' || b == 'o' || b == 'x')) {
      base = b == 'b' ? 2 : b == 'o' ? 8 : 16;
      i += 2;
    } else {
      base = 8;
      i += 1;
    }
  }
  const unsigned long long cutoff = base == 10 ? ~0ull / 10 + 1 : base == 16 ? 1ull << 60 : base == 8 ? 1ull << 61 : 1ull << 63;
  const unsigned long long max_val = bits == 64 ? ~0ull : (1ull << bits) - 1;
  unsigned long long n = 0;
  bool us_seen = false, us_bad = false;
  for (int64_t j = i; j < len; j += 8) {
    unsigned long long w = r.word(j);
    const int nb = len - j >= 8 ? 8 : (int)(len - j);
    for (int t = 0; t < nb; t++, w >>= 8) {
      const unsigned c = (unsigned)(w & 0xFF);
      unsigned d;
      if (c == '_') {
        us_seen = true;
        if (saw != '0') us_bad = true;
        saw = '_';
        continue;
      }
      if (c >= '0' && c <= '9') d = c - '0';
      else if ((c | 0x20) >= 'a' && (c | 0x20) <= 'z') d = (c | 0x20) - 'a' + 10;
      else return kScSyntax;
      if (d >= base) return kScSyntax;
      saw = '0';
      if (n >= cutoff) return kScRange;  // n · base overflows 64 bits
      n *= base;
      const unsigned long long n1 = n + d;
      if (n1 < n || n1 > max_val) return kScRange;
      n = n1;
    }
  }
  if (us_seen && (us_bad || saw == '_')) return kScSyntax;
  if (is_signed) {
    const unsigned long long half = 1ull << (bits - 1);
    if (!neg && n >= half) return kScRange;
    if (neg && n > half) return kScRange;
    if (neg) n = 0ull - n;
  }
  *out = n;
  return kScOk;
}

// strconv.ParseBool: exactly 1 t T TRUE true True → 1, 0 f F FALSE false False → 0; anything else a syntax error
template <class R>
AH_SC_FN int sc_parse_bool(const R& r, int* out) {
  *out = 0;
  const int64_t len = r.len;
  if (len != 1 && len != 4 && len != 5) return kScSyntax;
  const unsigned long long w = r.word(0);  // zero past the end: the length is part of the comparison
  if (len == 1) {
    if (w == '1' || w == 't' || w == 'T') { *out = 1; return kScOk; }
    return (w == '0' || w == 'f' || w == 'F') ? kScOk : kScSyntax;
  }
  if (len == 4) {
    if (w == 0x45555254ull /* TRUE */ || w == 0x65757274ull /* true */ || w == 0x65757254ull /* True */) { *out = 1; return kScOk; }
    return kScSyntax;
  }
  return (w == 0x45534C4146ull /* FALSE */ || w == 0x65736C6166ull /* false */ || w == 0x65736C6146ull /* False */) ? kScOk : kScSyntax;
}

// decimal digits of v: 1 … 20
AH_SC_FN int sc_digits_u64(unsigned long long v) {
  int d = 1;
  if (v >= 10000000000000000ull) { v /= 10000000000000000ull; d += 16; }
  if (v >= 100000000ull) { v /= 100000000ull; d += 8; }
  if (v >= 10000ull) { v /= 10000ull; d += 4; }
  if (v >= 100ull) { v /= 100ull; d += 2; }
  if (v >= 10ull) d += 1;
  return d;
}
// strconv.FormatInt(v, 10) / FormatUint(v, 10) of the 64-bit pattern `bits` (a signed value sign-extended): a minus sign, no plus,
// no leading zeros.  sc_format_len: the number of characters (1 … 20); sc_format_write: exactly those, to dst[0 … len).
AH_SC_FN int sc_format_len(unsigned long long bits, bool is_signed) {
  const bool neg = is_signed && (long long)bits < 0;
  return sc_digits_u64(neg ? 0ull - bits : bits) + (neg ? 1 : 0);
}
template <class P>
AH_SC_FN void sc_format_write(unsigned long long bits, bool is_signed, P dst, int len) {
  const bool neg = is_signed && (long long)bits < 0;
  unsigned long long m = neg ? 0ull - bits : bits;  // −2^63 is its own magnitude, 2^63, as an unsigned number
  for (int k = len - 1; k >= (neg ? 1 : 0); k--) {
    dst[k] = (uint8_t)('0' + (unsigned)(m % 10));
    m /= 10;
  }
  if (neg) dst[0] = '-';
}
// strconv.FormatBool: "true" / "false"
AH_SC_FN int sc_format_bool_len(int v) { return v ? 4 : 5; }
template <class P>
AH_SC_FN void sc_format_bool_write(int v, P dst) {
  const unsigned long long w = v ? 0x65757274ull : 0x65736C6166ull;
  for (int k = 0; k < (v ? 4 : 5); k++) dst[k] = (uint8_t)(w >> (8 * k));
}

// utf8.Valid over the sequences whose FIRST byte lies in [from, to) of the row (their continuation bytes may lie past `to`, never
// past the row).  from = 0, to = len is utf8.Valid of the row; a row cut into pieces is valid when every piece is: a piece that
// begins inside a sequence begun in the piece before skips the rest of that sequence, which the piece before checks — and a
// continuation byte no sequence accounts for is a first byte of its own, which fails.  Well-formed only: no overlong form, no
// surrogate, nothing above U+10FFFF, no truncated sequence.  A word of eight ASCII bytes takes one test.
template <class R>
AH_SC_FN bool sc_utf8_valid_range(const R& r, int64_t from, int64_t to) {
  const int64_t len = r.len;
  if (to > len) to = len;
  int64_t i = from;
  if (from > 0) {  // the last first-byte among the three bytes before `from`, and where its sequence ends
    const int64_t back = from >= 3 ? 3 : from;
    const unsigned long long w = r.word(from - back);
    for (int k = 1; k <= (int)back; k++) {
      const unsigned c = (unsigned)(w >> (8 * (back - k))) & 0xFF;
      if ((c & 0xC0) == 0x80) continue;
      const int need = c >= 0xF0 ? 4 : c >= 0xE0 ? 3 : c >= 0xC0 ? 2 : 1;
      if (need > k) i = from - k + need;
      break;
    }
  }
  while (i < to) {
    unsigned long long w = r.word(i);
    const unsigned long long high = w & 0x8080808080808080ull;
    if (high == 0) { i += 8; continue; }
    const int ascii = __builtin_ctzll(high) >> 3;  // ASCII bytes in front of the first one that is not
    if (ascii) { i += ascii; continue; }
    const unsigned c0 = (unsigned)w & 0xFF, c1 = (unsigned)(w >> 8) & 0xFF, c2 = (unsigned)(w >> 16) & 0xFF, c3 = (unsigned)(w >> 24) & 0xFF;
    // the second byte's range by the first (Go's acceptRanges); the zero a reader returns past the row's end is in none of them
    unsigned lo = 0x80, hi = 0xBF;
    int need;
    if (c0 >= 0xC2 && c0 <= 0xDF) need = 2;
    else if (c0 >= 0xE0 && c0 <= 0xEF) { need = 3; if (c0 == 0xE0) lo = 0xA0; if (c0 == 0xED) hi = 0x9F; }
    else if (c0 >= 0xF0 && c0 <= 0xF4) { need = 4; if (c0 == 0xF0) lo = 0x90; if (c0 == 0xF4) hi = 0x8F; }
    else return false;  // a continuation byte, C0 / C1, F5 … FF
    if (c1 < lo || c1 > hi) return false;
    if (need >= 3 && (c2 & 0xC0) != 0x80) return false;
    if (need == 4 && (c3 & 0xC0) != 0x80) return false;
    i += need;
  }
  return true;
}
template <class R>
AH_SC_FN bool sc_utf8_valid(const R& r) { return sc_utf8_valid_range(r, 0, r.len); }
