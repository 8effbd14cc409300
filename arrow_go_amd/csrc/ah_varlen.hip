// ah_varlen.hip — Take (and, through take indices, Filter) of binary / string columns: row §8(f)-4.
//
// Replaces VarBinaryImpl (arrow/compute/internal/kernels/vector_selection.go:1925-1992) driven by
// takeExec / filterExec (:1460-1598, 1821-1923) behind "array_take" / "array_filter" for
// Binary, String (int32 offsets) and LargeBinary, LargeString (int64 offsets):
//   a selected VALID slot appends the output offset and the value's bytes; every other emitted slot
//   (null value, null index, filter-null under EmitNulls) appends only the offset — a zero-length
//   null; output offsets start at 0; "binary output offset overflow" (checkBinaryTakeOffset
//   :1241-1247) when the bytes no longer fit the offset type; index bounds as in helpers.go:929-981.
// The reference appends value after value into growing builders.  Here the output size is data-
// dependent, so — like ah_filter_count / ah_filter_primitive — the work is two calls with the
// caller's allocation in between:
//   ah_take_binary_offsets  lengths gathered through the indices (+ validity word per 64 rows from a
//                           ballot, + fused bounds check) → scan (ah_scan.hip's kernels) → output
//                           offsets, total bytes, null count;
//   ah_take_binary_data     a wave owns 64 output rows: (source, destination, length) per lane,
//                           compacted through LDS; four 16-lane groups then copy four rows at a
//                           time, 4 (unaligned) bytes per lane.
// Filter = ah_filter_to_indices (GetTakeIndices, :102-236) + these two: filter(values, mask) and
// take(values, indices_of(mask)) select the same slots with the same validity, which is also how
// the reference filters record batches (compute/selection.go:687).
// Traffic: 2·w_off + w_idx read and w_off (+1/8) written per row in the first call (+ the scan's
// 24 B/row), the value bytes once in and once out in the second.
#include "ah_bytes.h"
#include "ah_index.h"
#include "ah_varout.h"

namespace {

constexpr int kBlock = 256;

// lens[i] = byte length of output row i (0 for a null), validity word per 64 rows, first out-of-bounds position
template <typename OffT, typename IdxT>
__global__ __launch_bounds__(kBlock) void lens_kernel(const OffT* __restrict__ offsets, const uint8_t* __restrict__ vvalid, int64_t voff,
                                                       unsigned long long nvalues, const IdxT* __restrict__ idx,
                                                       const uint8_t* __restrict__ ivalid, int64_t ioff, int64_t n,
                                                       long long* __restrict__ lens, uint8_t* __restrict__ out_valid,
                                                       unsigned long long* __restrict__ first_bad) {
  for_wave_chunks<kBlock>(n, [&](int64_t c, int64_t i) {
    const LaneIndex x = lane_index(idx, ivalid, ioff, i, n, vvalid, voff, nvalues, first_bad);
    if (i < n) lens[i] = x.ok ? (long long)offsets[voff + (int64_t)x.u + 1] - (long long)offsets[voff + (int64_t)x.u] : 0;
    if (out_valid) {
      const unsigned long long word = __ballot(x.ok);
      if (ah_lane() == 0) put_chunk_bytes(out_valid, c, n, word);
    }
  });
}

template <typename OffT, typename IdxT>
__global__ __launch_bounds__(kBlock) void copy_kernel(const OffT* __restrict__ offsets, const uint8_t* __restrict__ data, int64_t voff,
                                                       const IdxT* __restrict__ idx, int64_t n, const OffT* __restrict__ out_offsets,
                                                       uint8_t* __restrict__ out_data) {
  __shared__ CopyRow s_rows[kBlock / 64][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t c = (int64_t)blockIdx.x * (kBlock / 64) + wave; c < nchunks; c += wave_stride) {
    const int64_t i = c * 64 + lane;
    long long src = 0, dst = 0, len = 0;
    if (i < n) {
      dst = (long long)out_offsets[i];
      len = (long long)out_offsets[i + 1] - dst;
      if (len > 0) src = (long long)offsets[voff + (int64_t)idx[i]];  // len > 0 ⇒ a valid, in-bounds slot (IdxT is unsigned)
    }
    wave_copy_rows(s_rows[wave], data + src, out_data + dst, len);   // (ah_bytes.h)
  }
}


template <typename OffT, typename IdxT>
int run_lens(ah_ctx* c, const void* offsets, const uint8_t* vvalid, int64_t voff, int64_t nvalues, const void* idx, const uint8_t* ivalid,
             int64_t ioff, int64_t n, uint8_t* out_valid, long long* lens) {
  const unsigned grid = ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, 64), kBlock / 64), 8);
  lens_kernel<OffT, IdxT><<<grid, kBlock, 0, c->stream>>>((const OffT*)offsets, vvalid, voff, (unsigned long long)nvalues, (const IdxT*)idx, ivalid,
                                                         ioff, n, lens, out_valid, (unsigned long long*)&c->dscalars[kDsVarFirst]);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

template <typename OffT>
int run_copy(ah_ctx* c, int iw, const void* offsets, const uint8_t* data, int64_t voff, const void* idx, int64_t n, const void* out_offsets,
             uint8_t* out_data) {
  const unsigned grid = ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, 64), kBlock / 64), 16);
  const bool known = with_index_type(iw, /*is_signed=*/0, [&](auto it) {
    using IdxT = typename std::make_unsigned<typename decltype(it)::type>::type;   // the unsigned reinterpretation is all the copy needs
    copy_kernel<OffT, IdxT><<<grid, kBlock, 0, c->stream>>>((const OffT*)offsets, data, voff, (const IdxT*)idx, n, (const OffT*)out_offsets, out_data);
  });
  if (!known) return ah_fail(c, AH_EINDEX, "invalid indices byte width");
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

}  // namespace

AH_EXPORT int ah_take_binary_offsets(ah_ctx* c, int offset_width, const void* offsets, const uint8_t* vvalid, int64_t voff, int64_t nvalues,
                                     int idx_byte_width, int idx_signed, const void* idx, const uint8_t* ivalid, int64_t ioff, int64_t nidx,
                                     int bounds_check, void* out_offsets, uint8_t* out_valid, int64_t* out_null_count_host,
                                     int64_t* out_total_bytes_host, int64_t* bad_index_host) {
  AH_ENTER(c);
  (void)bounds_check;  // fused and always on, like ah_take_primitive
  if (out_total_bytes_host) *out_total_bytes_host = 0;
  int rc = take_enter(c, nidx, nvalues, voff, ioff, out_offsets && offsets && (nidx == 0 || idx), out_valid, &vvalid, &ivalid, out_null_count_host);
  if (rc != AH_OK) return rc;
  if (offset_width != 4 && offset_width != 8) return ah_fail(c, AH_EINVALID, "take: binary offsets are 4 or 8 bytes wide");
  if (nidx == 0) {  // a lone closing offset
    AH_HIP(c, hipMemsetAsync(out_offsets, 0, (size_t)offset_width, c->stream));
    return AH_OK;
  }
  VarOut v;
  rc = varout_begin(c, nidx, 0, /*can_overflow=*/true, &v);   // (zeroes the valid count and the overflow flag)
  if (rc != AH_OK) return rc;
  AH_HIP(c, hipMemsetAsync(&c->dscalars[kDsVarFirst], 0xFF, sizeof(uint64_t), c->stream));  // first bad position
  const bool known = with_index_type(idx_byte_width, idx_signed, [&](auto it) {
    using IdxT = typename decltype(it)::type;
    rc = offset_width == 4 ? run_lens<int32_t, IdxT>(c, offsets, vvalid, voff, nvalues, idx, ivalid, ioff, nidx, out_valid, v.lens)
                           : run_lens<int64_t, IdxT>(c, offsets, vvalid, voff, nvalues, idx, ivalid, ioff, nidx, out_valid, v.lens);
  });
  if (!known) return ah_fail(c, AH_EINDEX, "invalid indices byte width");
  if (rc != AH_OK) return rc;
  if (out_valid && out_null_count_host) {
    rc = ah_popcount_async(c, out_valid, 0, nidx, (unsigned long long*)&c->dscalars[kDsVarCount]);
    if (rc != AH_OK) return rc;
  }
  rc = varout_enqueue(c, v, nidx, offset_width, out_offsets, /*caller_words=*/true);
  if (rc != AH_OK) return rc;
  int64_t total = 0;
  bool overflow = false;
  rc = varout_finish(c, v, &total, &overflow);
  if (rc != AH_OK) return rc;
  const uint64_t bad_pos = *(volatile uint64_t*)&c->pinned[kVarPinFirst];
  const uint64_t nvalid = *(volatile uint64_t*)&c->pinned[kVarPinCount];
  if (bad_pos != ~0ull) return take_fail_bad_index(c, idx, idx_byte_width, idx_signed, bad_pos, bad_index_host);
  if (overflow) return ah_fail(c, AH_EINVALID, "binary output offset overflow");  // :1245
  if (out_null_count_host) *out_null_count_host = out_valid ? nidx - (int64_t)nvalid : 0;
  if (out_total_bytes_host) *out_total_bytes_host = total;
  return AH_OK;
}

AH_EXPORT int ah_take_binary_data(ah_ctx* c, int offset_width, const void* offsets, const uint8_t* data, int64_t voff, int idx_byte_width,
                                  const void* idx, int64_t nidx, const void* out_offsets, uint8_t* out_data) {
  AH_ENTER(c);
  if (nidx < 0 || voff < 0) return ah_fail(c, AH_EINVALID, "take: negative length/offset");
  if (offset_width != 4 && offset_width != 8) return ah_fail(c, AH_EINVALID, "take: binary offsets are 4 or 8 bytes wide");
  if (nidx == 0) return AH_OK;
  if (!offsets || !idx || !out_offsets) return ah_fail(c, AH_EINVALID, "take: null buffer");
  return offset_width == 4 ? run_copy<int32_t>(c, idx_byte_width, offsets, data, voff, idx, nidx, out_offsets, out_data)
                           : run_copy<int64_t>(c, idx_byte_width, offsets, data, voff, idx, nidx, out_offsets, out_data);
}
