// decimal_harness.cc — csrc/ah_decimal.h compiled for the host: each limb routine over `count` rows of `limbs` 64-bit words
// (tests/test_decimal_host.py compares them with Python integers).
#include "../arrow_go_amd/csrc/ah_decimal.h"

#include <cstring>

namespace {

template <int N>
void mul_rows(const unsigned long long* in, long count, const int* k, unsigned long long* out, unsigned char* carry) {
  for (long i = 0; i < count; i++) {
    unsigned long long w[N];
    memcpy(w, in + i * N, sizeof w);
    carry[i] = dec_mul_pow10<N>(w, k[i]) ? 1 : 0;
    memcpy(out + i * N, w, sizeof w);
  }
}

template <int N>
void div_rows(const unsigned long long* in, long count, const int* k, unsigned long long* out, unsigned char* nonzero, unsigned char* half) {
  for (long i = 0; i < count; i++) {
    unsigned long long x[N], q[N];
    memcpy(x, in + i * N, sizeof x);
    bool nz = false, hf = false, nz2 = false, unused = false;
    dec_div_pow10<N, true>(x, k[i], q, &nz, &hf);
    unsigned long long q2[N];
    dec_div_pow10<N, false>(x, k[i], q2, &nz2, &unused);   // the variant without the half test: same quotient, same remainder test
    if (memcmp(q, q2, sizeof q) != 0 || nz != nz2) { nz = !nz; q[0] = ~q[0]; }
    nonzero[i] = nz;
    half[i] = hf;
    memcpy(out + i * N, q, sizeof q);
  }
}

template <int N>
void unary_rows(int op, const unsigned long long* in, long count, unsigned long long* out, unsigned char* flag) {
  for (long i = 0; i < count; i++) {
    unsigned long long w[N];
    memcpy(w, in + i * N, sizeof w);
    flag[i] = dec_is_negative<N>(w) ? 1 : 0;
    if (op == 0) dec_negate<N>(w);
    else dec_increment<N>(w);
    memcpy(out + i * N, w, sizeof w);
  }
}

template <int N>
void less_rows(const unsigned long long* a, const unsigned long long* b, long count, unsigned char* out) {
  for (long i = 0; i < count; i++) {
    unsigned long long x[N], y[N];
    memcpy(x, a + i * N, sizeof x);
    memcpy(y, b + i * N, sizeof y);
    out[i] = dec_fits_precision<N>(x, y) ? 1 : 0;
  }
}

}  // namespace

extern "C" {

void dh_mul_pow10(int limbs, const unsigned long long* in, long count, const int* k, unsigned long long* out, unsigned char* carry) {
  if (limbs == 2) mul_rows<2>(in, count, k, out, carry);
  else mul_rows<4>(in, count, k, out, carry);
}

void dh_div_pow10(int limbs, const unsigned long long* in, long count, const int* k, unsigned long long* out, unsigned char* nonzero,
                  unsigned char* half) {
  if (limbs == 2) div_rows<2>(in, count, k, out, nonzero, half);
  else div_rows<4>(in, count, k, out, nonzero, half);
}

// op 0: negate, 1: increment; flag = the sign of the input
void dh_unary(int limbs, int op, const unsigned long long* in, long count, unsigned long long* out, unsigned char* flag) {
  if (limbs == 2) unary_rows<2>(op, in, count, out, flag);
  else unary_rows<4>(op, in, count, out, flag);
}

void dh_fits(int limbs, const unsigned long long* mag, const unsigned long long* bound, long count, unsigned char* out) {
  if (limbs == 2) less_rows<2>(mag, bound, count, out);
  else less_rows<4>(mag, bound, count, out);
}

// the comparisons' scale_up (I256, modulo 2^256)
void dh_scale_up(const unsigned long long* in, long count, const int* k, unsigned long long* out) {
  for (long i = 0; i < count; i++) {
    I256 x;
    memcpy(x.w, in + i * 4, sizeof x.w);
    scale_up(x, k[i]);
    memcpy(out + i * 4, x.w, sizeof x.w);
  }
}
}
