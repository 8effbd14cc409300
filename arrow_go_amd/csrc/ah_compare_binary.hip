// ah_compare_binary.hip — equal / not_equal / greater / greater_equal of byte strings and decimals → packed bitmap.
//
// Replaces the base-binary, FixedSizeBinary and decimal kernels of CompareKernels (arrow/compute/internal/kernels/
// scalar_comparisons.go:694-713: getBinaryCmp :520-540 over NewVarBinaryIter / NewFSBIter, genDecimalCompareKernel
// :370-392) behind compute's "equal", "not_equal", "greater", "greater_equal" (+ "less" / "less_equal" by operand swap,
// compute/scalar_compare.go:73-99).
//
// Byte strings (bytes.Equal / bytes.Compare: unsigned, bytewise, a proper prefix first).  Each operand is a ByteRows column
// (ah_bytes.h) — 4- or 8-byte offsets + data, or fixed slots of byte_width bytes — so String ∘ LargeBinary, FixedSizeBinary[3] ∘
// FixedSizeBinary[1] and FixedSizeBinary ∘ String compare as they are, with no cast.  One row per lane, one ballot per
// 64 rows, written as one 64-bit word.  equal / not_equal decide from the two lengths first: only rows of equal length
// read bytes.  Ordering compares byte-swapped 8-byte words; the first word that differs decides, else the lengths do.
// A lane compares at most kLaneCmp bytes itself; a row whose common prefix goes further is handed to the whole wave,
// which compares 512 bytes per step (64 lanes × 8 bytes), one pending row after another — a 4 KiB value does not
// serialise its 63 neighbours (wave_compare of ah_bytes.h, shared with is_in).  A broadcast (scalar) operand is read once per
// workgroup into LDS when it is at most kScalarLds bytes, else read from global memory.  The word orders (order_words,
// order_range) are ah_bytes.h's; the result word is stored by put_word (ah_common.h).
//
// Decimals: one 16- or 32-byte load per row, sign-extended to 256 bits, multiplied by 10^k (the side's scale-up, from a
// table of 64-bit powers of ten) and compared as signed two's complement: top word signed, lower words unsigned.
#include "ah_common.h"
#include "ah_bytes.h"
#include "ah_decimal.h"

namespace {

constexpr int kBlock = 256;
constexpr int64_t kLaneFast = 64;  // bytes of the lane's first, unrolled compare (random keys decide here)
constexpr int64_t kLaneCmp = 256;  // bytes a lane compares on its own (32 words: a 65-byte shared prefix stays lane-local)
constexpr int kScalarLds = 4096;  // a broadcast value up to this many bytes is staged in LDS

// a broadcast operand's value: into `lds` when it fits (every thread of the block calls this)
template <int OW>
__device__ __forceinline__ void stage(const ByteRows& s, uint8_t* lds, const uint8_t** p, int64_t* len) {
  row_at<OW>(s, 0, p, len);
  if (*len <= kScalarLds) {
    for (int64_t j = threadIdx.x; j < *len; j += kBlock) lds[j] = (*p)[j];
    *p = lds;
  }
}

__device__ __forceinline__ bool decide(int op, int c) {
  return op == AH_CMP_EQ ? c == 0 : op == AH_CMP_NE ? c != 0 : op == AH_CMP_GT ? c > 0 : c >= 0;
}

template <int OWL, int OWR>
__global__ __launch_bounds__(kBlock) void compare_bytes_kernel(ByteRows L, ByteRows R, int l_bcast, int r_bcast, int op, int64_t n,
                                                               uint8_t* __restrict__ out, int64_t out_off, int aligned) {
  __shared__ unsigned long long s_l[kScalarLds / 8], s_r[kScalarLds / 8];  // 8-byte aligned: staged values are read in words
  const uint8_t* lp = nullptr;
  const uint8_t* rp = nullptr;
  int64_t ll = 0, lr = 0;
  if (l_bcast) stage<OWL>(L, (uint8_t*)s_l, &lp, &ll);
  if (r_bcast) stage<OWR>(R, (uint8_t*)s_r, &rp, &lr);
  if (l_bcast || r_bcast) __syncthreads();
  const bool eq_op = op == AH_CMP_EQ || op == AH_CMP_NE;
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const int cnt = left >= 64 ? 64 : (int)left;
    const bool active = lane < cnt;
    const uint8_t* a = lp;
    const uint8_t* b = rp;
    int64_t la = ll, lb = lr;
    int c = 0;
    bool pend = false;
    int64_t m = 0;
    if (active) {
      if (!l_bcast) row_at<OWL>(L, row, &a, &la);
      if (!r_bcast) row_at<OWR>(R, row, &b, &lb);
      m = la < lb ? la : lb;
      if (eq_op && la != lb) {
        c = 1;
      } else {
        c = order_range(a, b, 0, m < kLaneFast ? m : kLaneFast);
        if (c == 0) {
          if (m > kLaneFast) pend = true;
          else c = (la > lb) - (la < lb);
        }
      }
    }
    unsigned long long need = __ballot(pend);
    if (need) {  // rows whose first kLaneFast bytes tie: each lane goes on alone up to kLaneCmp
      if (pend) {
        c = order_range(a, b, kLaneFast, m < kLaneCmp ? m : kLaneCmp);
        if (c != 0 || m <= kLaneCmp) {
          if (c == 0) c = (la > lb) - (la < lb);
          pend = false;
        }
      }
      need = __ballot(pend);
    }
    // rows whose first kLaneCmp bytes tie and go on: the wave compares the rest, 512 bytes per step
    wave_compare<true>(need, a, b, m, kLaneCmp, [&](int r) { c = r != 0 ? r : (la > lb) - (la < lb); });
    const unsigned long long word = __ballot(active && decide(op, c));
    if (lane == 0) put_word(out, out_off, aligned, ch, word, cnt);
  }
}

// ---- decimals ---------------------------------------------------------------------------------------------------------------
// I256, kPow10, load_dec and scale_up: ah_decimal.h
__device__ __forceinline__ int order_i256(const I256& a, const I256& b) {
  if (a.w[3] != b.w[3]) return (long long)a.w[3] < (long long)b.w[3] ? -1 : 1;
#pragma unroll
  for (int t = 2; t >= 0; t--)
    if (a.w[t] != b.w[t]) return a.w[t] < b.w[t] ? -1 : 1;
  return 0;
}

template <int WL, int WR>
__global__ __launch_bounds__(kBlock) void compare_decimal_kernel(const uint8_t* __restrict__ l, int l_bcast, int kl, const uint8_t* __restrict__ r,
                                                                 int r_bcast, int kr, int op, int64_t n, uint8_t* __restrict__ out,
                                                                 int64_t out_off, int aligned) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const int cnt = left >= 64 ? 64 : (int)left;
    bool bit = false;
    if (lane < cnt) {
      I256 a = load_dec<WL>(l + (l_bcast ? 0 : row * WL));
      I256 b = load_dec<WR>(r + (r_bcast ? 0 : row * WR));
      if (kl) scale_up(a, kl);
      if (kr) scale_up(b, kr);
      bit = decide(op, order_i256(a, b));
    }
    const unsigned long long word = __ballot(bit);
    if (lane == 0) put_word(out, out_off, aligned, ch, word, cnt);
  }
}

int check_out(ah_ctx* c, int cmpop, int64_t n, uint8_t* out, int64_t out_off) {
  if (n < 0 || out_off < 0) return ah_fail(c, AH_EINVALID, "comparison: negative length/offset");
  if (cmpop < AH_CMP_EQ || cmpop > AH_CMP_GE) return ah_fail(c, AH_EINVALID, "comparison: bad op %d", cmpop);
  if (n > 0 && !out) return ah_fail(c, AH_EINVALID, "comparison: null output bitmap");
  return AH_OK;
}

unsigned chunk_grid(ah_ctx* c, int64_t n) { return ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, 64), kBlock / 64), 8); }

int out_aligned(const uint8_t* out, int64_t out_off) { return (out_off & 63) == 0 && ((uintptr_t)out & 7) == 0; }

template <int OWL, int OWR>
void launch_bytes(ah_ctx* c, const ah_cmp_operand* l, const ah_cmp_operand* r, int op, int64_t n, uint8_t* out, int64_t out_off) {
  compare_bytes_kernel<OWL, OWR><<<chunk_grid(c, n), kBlock, 0, c->stream>>>(
      byte_rows(OWL, l->offsets, l->data, l->byte_width, l->off), byte_rows(OWR, r->offsets, r->data, r->byte_width, r->off), l->broadcast ? 1 : 0,
      r->broadcast ? 1 : 0, op, n, out, out_off, out_aligned(out, out_off));
}

template <int OWL>
void launch_bytes_r(ah_ctx* c, const ah_cmp_operand* l, const ah_cmp_operand* r, int op, int64_t n, uint8_t* out, int64_t out_off) {
  if (r->offset_width == 4) launch_bytes<OWL, 4>(c, l, r, op, n, out, out_off);
  else if (r->offset_width == 8) launch_bytes<OWL, 8>(c, l, r, op, n, out, out_off);
  else launch_bytes<OWL, 0>(c, l, r, op, n, out, out_off);
}

template <int WL, int WR>
void launch_decimal(ah_ctx* c, const uint8_t* l, int lb, int kl, const uint8_t* r, int rb, int kr, int op, int64_t n, uint8_t* out, int64_t out_off) {
  compare_decimal_kernel<WL, WR><<<chunk_grid(c, n), kBlock, 0, c->stream>>>(l, lb, kl, r, rb, kr, op, n, out, out_off, out_aligned(out, out_off));
}

}  // namespace

AH_EXPORT int ah_compare_binary(ah_ctx* c, int cmpop, const ah_cmp_operand* l, const ah_cmp_operand* r, int64_t n, uint8_t* out_bits,
                                int64_t out_bit_offset) {
  AH_ENTER(c);
  int rc = check_out(c, cmpop, n, out_bits, out_bit_offset);
  if (rc != AH_OK) return rc;
  if (!l || !r) return ah_fail(c, AH_EINVALID, "comparison: null operand descriptor");
  const ah_cmp_operand* ops[2] = {l, r};
  for (const ah_cmp_operand* o : ops) {
    if (o->offset_width != 0 && o->offset_width != 4 && o->offset_width != 8)
      return ah_fail(c, AH_EINVALID, "comparison: offset width must be 0, 4 or 8 (got %d)", o->offset_width);
    if (o->offset_width == 0 && o->byte_width < 0) return ah_fail(c, AH_EINVALID, "comparison: negative byte width");
    if (o->off < 0) return ah_fail(c, AH_EINVALID, "comparison: negative element offset");
  }
  if (n == 0) return AH_OK;
  for (const ah_cmp_operand* o : ops) {
    if (o->offset_width != 0 && !o->offsets) return ah_fail(c, AH_EINVALID, "comparison: null offsets");
    if (!o->data && o->offset_width == 0 && o->byte_width > 0) return ah_fail(c, AH_EINVALID, "comparison: null data");
  }
  if (l->offset_width == 4) launch_bytes_r<4>(c, l, r, cmpop, n, out_bits, out_bit_offset);
  else if (l->offset_width == 8) launch_bytes_r<8>(c, l, r, cmpop, n, out_bits, out_bit_offset);
  else launch_bytes_r<0>(c, l, r, cmpop, n, out_bits, out_bit_offset);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

AH_EXPORT int ah_compare_decimal(ah_ctx* c, int cmpop, int l_width, const uint8_t* l, int64_t l_off, int l_broadcast, int l_scaleup, int r_width,
                                 const uint8_t* r, int64_t r_off, int r_broadcast, int r_scaleup, int64_t n, uint8_t* out_bits,
                                 int64_t out_bit_offset) {
  AH_ENTER(c);
  int rc = check_out(c, cmpop, n, out_bits, out_bit_offset);
  if (rc != AH_OK) return rc;
  if ((l_width != 16 && l_width != 32) || (r_width != 16 && r_width != 32))
    return ah_fail(c, AH_EINVALID, "comparison: decimal width must be 16 or 32 (got %d, %d)", l_width, r_width);
  if (l_off < 0 || r_off < 0) return ah_fail(c, AH_EINVALID, "comparison: negative element offset");
  if (l_scaleup < 0 || l_scaleup > 76 || r_scaleup < 0 || r_scaleup > 76)
    return ah_fail(c, AH_EINVALID, "comparison: decimal scale-up must be 0 … 76 (got %d, %d)", l_scaleup, r_scaleup);
  if (n == 0) return AH_OK;
  if (!l || !r) return ah_fail(c, AH_EINVALID, "comparison: null buffer");
  const uint8_t* lp = l + l_off * l_width;
  const uint8_t* rp = r + r_off * r_width;
  const int lb = l_broadcast ? 1 : 0, rb = r_broadcast ? 1 : 0;
  if (l_width == 16 && r_width == 16) launch_decimal<16, 16>(c, lp, lb, l_scaleup, rp, rb, r_scaleup, cmpop, n, out_bits, out_bit_offset);
  else if (l_width == 16) launch_decimal<16, 32>(c, lp, lb, l_scaleup, rp, rb, r_scaleup, cmpop, n, out_bits, out_bit_offset);
  else if (r_width == 16) launch_decimal<32, 16>(c, lp, lb, l_scaleup, rp, rb, r_scaleup, cmpop, n, out_bits, out_bit_offset);
  else launch_decimal<32, 32>(c, lp, lb, l_scaleup, rp, rb, r_scaleup, cmpop, n, out_bits, out_bit_offset);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}
