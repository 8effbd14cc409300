// ah_cast_string.hip — the string casts: String / Binary → integer and boolean (parse), integer and boolean → String (format),
// UTF-8 validation of Binary / FixedSizeBinary columns cast to String, and the offsets of FixedSizeBinary → Binary.
//
// Replaces getParseStringExec under ScalarUnaryNotNullBinaryArg (arrow/compute/internal/kernels/numeric_cast.go:742-781,
// helpers.go:130-154), the ParseBool kernels (boolean_cast.go:77-95), the numeric → string formatters of
// addNumericAndTemporalToStringCasts (string_casts.go), validateUTF8Sequence (string_casts.go:39-87) and the offsets loop of
// CastFsbToBinary (string_casts.go:154-193) behind compute's "cast".  The rules themselves are ah_strconv.h; rows are found with
// ah_bytes.h.
//
//   parse      one row per lane, 8-byte loads inside the row.  A null row is not read and gives 0.  The reference overwrites its error
//              row after row, so the call's error is that of the LAST offending valid row: atomicMax of (row + 1) · 4 + kind.
//              Boolean output: one ballot per 64 rows, stored as a word.
//   format     two calls with the caller's allocation in between, like ah_take_binary_offsets / _data: lengths → the scan of
//              ah_scan.hip → offsets and the byte total; then a workgroup formats 256 rows into LDS, laid out as the output is
//              aligned, and writes the stretch in 16-byte words (single bytes only at its two ends).
//   validate   utf8.Valid per valid row, the FIRST offender by atomicMin.  Rows up to 64 bytes stay on their lane; longer ones are
//              taken by the whole wave one after the other, 16 bytes per lane and step (sc_utf8_valid_range).
#include "ah_bytes.h"
#include "ah_strconv.h"
#include "ah_varout.h"

namespace {

constexpr int kBlock = 256;
constexpr int kLongRow = 64;   // validate: bytes a lane checks alone
constexpr int kPiece = 16;     // … and bytes per lane and step of a row the wave shares
constexpr int kMaxChars = 20;  // "-9223372036854775808", "18446744073709551615"

struct DevRow {  // ah_strconv.h's reader: 8 bytes at i, zero past the row's end
  const uint8_t* p;
  int64_t len;
  __device__ __forceinline__ unsigned long long word(int64_t i) const { return word_at(p, i, len); }
};

// String → integer of B bytes
template <int OW, int B>
__global__ __launch_bounds__(kBlock) void parse_int_kernel(ByteRows rows, const uint8_t* __restrict__ valid, int64_t off, int64_t n, int is_signed,
                                                           uint8_t* __restrict__ out, unsigned long long* __restrict__ last_bad) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  unsigned long long bad_at = 0;
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const unsigned long long vword = valid ? ah_wave_bits64(valid, off + ch * 64, left) : ~0ull;
    if (lane >= left) continue;
    unsigned long long v = 0;
    if ((vword >> lane) & 1) {
      DevRow r;
      row_at<OW>(rows, row, &r.p, &r.len);
      const int kind = sc_parse_int(r, B * 8, is_signed != 0, &v);
      if (kind) {
        v = 0;
        const unsigned long long at = ((unsigned long long)(row + 1) << 2) | (unsigned)kind;
        if (at > bad_at) bad_at = at;
      }
    }
    uint8_t* o = out + row * B;
    if constexpr (B == 1) *o = (uint8_t)v;
    else if constexpr (B == 2) *(uint16_t*)o = (uint16_t)v;
    else if constexpr (B == 4) *(uint32_t*)o = (uint32_t)v;
    else *(unsigned long long*)o = v;
  }
  if (bad_at) atomicMax(last_bad, bad_at);
}

// String → boolean: a bitmap from bit 0, one word per 64 rows
template <int OW>
__global__ __launch_bounds__(kBlock) void parse_bool_kernel(ByteRows rows, const uint8_t* __restrict__ valid, int64_t off, int64_t n,
                                                            uint8_t* __restrict__ out_bits, int out_aligned, unsigned long long* __restrict__ last_bad) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  unsigned long long bad_at = 0;
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const unsigned long long vword = valid ? ah_wave_bits64(valid, off + ch * 64, left) : ~0ull;
    int v = 0;
    if (lane < left && ((vword >> lane) & 1)) {
      DevRow r;
      row_at<OW>(rows, row, &r.p, &r.len);
      const int kind = sc_parse_bool(r, &v);
      if (kind) {
        const unsigned long long at = ((unsigned long long)(row + 1) << 2) | (unsigned)kind;
        if (at > bad_at) bad_at = at;
      }
    }
    const unsigned long long word = __ballot(v != 0);
    if (lane == 0) {
      if (out_aligned && left >= 64) *(unsigned long long*)(out_bits + ch * 8) = word;
      else put_chunk_bytes(out_bits, ch, n, word);
    }
  }
  if (bad_at) atomicMax(last_bad, bad_at);
}

// row i of an integer column of B bytes as a 64-bit pattern, sign- or zero-extended
template <int B>
__device__ __forceinline__ unsigned long long load_int(const uint8_t* __restrict__ in, int64_t i, int is_signed) {
  if constexpr (B == 1) return is_signed ? (unsigned long long)(long long)((const int8_t*)in)[i] : in[i];
  else if constexpr (B == 2) return is_signed ? (unsigned long long)(long long)((const int16_t*)in)[i] : ((const uint16_t*)in)[i];
  else if constexpr (B == 4) return is_signed ? (unsigned long long)(long long)((const int32_t*)in)[i] : ((const uint32_t*)in)[i];
  else return ((const unsigned long long*)in)[i];
}

// lens[i] = characters of row i, 0 for a null.  B = 0: a boolean column, the data bitmap read at bit `off` like the validity.
template <int B>
__global__ __launch_bounds__(kBlock) void format_lens_kernel(const uint8_t* __restrict__ in, const uint8_t* __restrict__ valid, int64_t off, int64_t n,
                                                             int is_signed, long long* __restrict__ lens) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const unsigned long long vword = valid ? ah_wave_bits64(valid, off + ch * 64, left) : ~0ull;
    unsigned long long dword = 0;
    if constexpr (B == 0) dword = ah_wave_bits64(in, off + ch * 64, left);
    if (lane >= left) continue;
    int len = 0;
    if ((vword >> lane) & 1) {
      if constexpr (B == 0) len = sc_format_bool_len((int)((dword >> lane) & 1));
      else len = sc_format_len(load_int<B>(in, row, is_signed), is_signed != 0);
    }
    lens[row] = len;
  }
}

// The characters.  A workgroup takes 256 rows at a time: their bytes are one stretch [offsets[r0], offsets[r0 + rows]) of the output.
// Every lane formats its row into LDS at the position the byte has in the output relative to the 16-byte boundary at or below the
// stretch's start; the workgroup then copies whole 16-byte words LDS → global and the bytes of the partial words at the two ends.
template <int B, typename OffT>
__global__ __launch_bounds__(kBlock) void format_data_kernel(const uint8_t* __restrict__ in, const uint8_t* __restrict__ valid, int64_t off, int64_t n,
                                                             int is_signed, const OffT* __restrict__ offsets, uint8_t* __restrict__ out_data) {
  __shared__ uint4 s_words[(kBlock * kMaxChars + 16) / 16 + 1];
  uint8_t* s_bytes = (uint8_t*)s_words;
  const int lane = threadIdx.x & 63;
  const int64_t ntiles = (n + kBlock - 1) / kBlock;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * kBlock;
    const int64_t rows = n - r0 < kBlock ? n - r0 : kBlock;
    const int64_t row = r0 + threadIdx.x;
    const int64_t left = n - (r0 + (threadIdx.x & ~63));  // rows from this wave's lane 0 on
    const int64_t start = (int64_t)offsets[r0], end = (int64_t)offsets[r0 + rows];
    if (end < start || end - start > kBlock * kMaxChars) continue;  // offsets that are not this column's: nothing is written (block-uniform)
    const int lead = (int)(((uintptr_t)out_data + (uintptr_t)start) & 15);  // the stretch's first byte within its 16-byte word
    const uint8_t* base = out_data + start - lead;                          // 16-byte aligned; only bytes from `start` on are written
    unsigned long long vword = 0, dword = 0;
    if (left > 0) {
      vword = valid ? ah_wave_bits64(valid, off + row - lane, left) : ~0ull;
      if constexpr (B == 0) dword = ah_wave_bits64(in, off + row - lane, left);
    }
    if (row < n && ((vword >> lane) & 1)) {
      const int64_t at = (int64_t)offsets[row] - start;
      unsigned long long v = 0;
      int len;
      if constexpr (B == 0) len = sc_format_bool_len((int)((dword >> lane) & 1));
      else { v = load_int<B>(in, row, is_signed); len = sc_format_len(v, is_signed != 0); }
      if (at >= 0 && at + len <= end - start) {  // always, with the offsets ah_format_int_offsets made of this column
        uint8_t* dst = s_bytes + lead + at;
        if constexpr (B == 0) sc_format_bool_write((int)((dword >> lane) & 1), dst);
        else sc_format_write(v, is_signed != 0, dst, len);
      }
    }
    __syncthreads();
    const int endl = lead + (int)(end - start);            // the stretch in LDS: [lead, endl)
    const int first_word = (lead + 15) >> 4, last_word = endl >> 4;  // whole words: [first_word, last_word)
    uint8_t* gbase = const_cast<uint8_t*>(base);
    for (int w = first_word + (int)threadIdx.x; w < last_word; w += kBlock) *(uint4*)(gbase + (int64_t)w * 16) = s_words[w];
    const int head_end = first_word * 16 < endl ? first_word * 16 : endl;
    const int tail_begin = last_word * 16 > head_end ? last_word * 16 : head_end;
    for (int b = lead + (int)threadIdx.x; b < head_end; b += kBlock) gbase[b] = s_bytes[b];
    for (int b = tail_begin + (int)threadIdx.x; b < endl; b += kBlock) gbase[b] = s_bytes[b];
    __syncthreads();  // the next tile overwrites the staging area
  }
}

// utf8.Valid of every valid row; the smallest offending row wins
template <int OW>
__global__ __launch_bounds__(kBlock) void validate_utf8_kernel(ByteRows rows, const uint8_t* __restrict__ valid, int64_t off, int64_t n,
                                                               unsigned long long* __restrict__ first_bad) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  unsigned long long bad_at = ~0ull;
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const unsigned long long vword = valid ? ah_wave_bits64(valid, off + ch * 64, left) : ~0ull;
    DevRow r{nullptr, 0};
    const bool live = lane < left && ((vword >> lane) & 1);
    if (live) row_at<OW>(rows, row, &r.p, &r.len);
    bool bad = false;
    if (live && r.len <= kLongRow) bad = !sc_utf8_valid(r);
    // long rows: the whole wave, one pending lane after another (all 64 lanes are here: nothing above leaves the loop body)
    unsigned long long need = __ballot(live && r.len > kLongRow);
    while (need) {
      const int l = __ffsll((long long)need) - 1;
      need &= need - 1;
      DevRow w;
      w.p = (const uint8_t*)(uintptr_t)__shfl((long long)(uintptr_t)r.p, l);
      w.len = __shfl((long long)r.len, l);
      bool piece_bad = false;
      for (int64_t from = (int64_t)lane * kPiece; from < w.len; from += 64 * kPiece) piece_bad |= !sc_utf8_valid_range(w, from, from + kPiece);
      const bool any = __ballot(piece_bad) != 0ull;
      if (lane == l) bad = any;
    }
    if (bad && (unsigned long long)row < bad_at) bad_at = (unsigned long long)row;
  }
  if (bad_at != ~0ull) atomicMin(first_bad, bad_at);
}

// FixedSizeBinary → Binary: offsets[i] = (off + i) · width, i = 0 … n
template <typename OffT>
__global__ __launch_bounds__(kBlock) void fixed_offsets_kernel(int64_t off, int64_t width, int64_t n, OffT* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i <= n; i += stride) out[i] = (OffT)((off + i) * width);
}

unsigned chunk_grid(ah_ctx* c, int64_t n) { return ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, 64), kBlock / 64), 8); }

unsigned long long* bad_word(ah_ctx* c) { return (unsigned long long*)&c->dscalars[12]; }

int arm_bad(ah_ctx* c, int byte_value) {
  AH_HIP(c, hipMemsetAsync(bad_word(c), byte_value, sizeof(uint64_t), c->stream));
  return AH_OK;
}
int read_bad(ah_ctx* c, unsigned long long* at) {
  AH_HIP(c, hipMemcpyAsync(c->pinned, bad_word(c), sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipStreamSynchronize(c->stream));
  *at = *(volatile unsigned long long*)c->pinned;
  return AH_OK;
}

// bytes and signedness of an integer type id; AH_BOOL: 0 bytes
bool format_type(int t, int* bytes, int* is_signed) {
  switch (t) {
    case AH_BOOL: *bytes = 0; *is_signed = 0; return true;
    case AH_UINT8: case AH_UINT16: case AH_UINT32: case AH_UINT64: *is_signed = 0; *bytes = ah_type_width(t); return true;
    case AH_INT8: case AH_INT16: case AH_INT32: case AH_INT64: *is_signed = 1; *bytes = ah_type_width(t); return true;
  }
  return false;
}

int check_rows(ah_ctx* c, const char* what, int offset_width, const void* offsets, int64_t off, int64_t n) {
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "%s: negative length/offset", what);
  if (offset_width != 4 && offset_width != 8) return ah_fail(c, AH_EINVALID, "%s: binary offsets are 4 or 8 bytes wide", what);
  if (n > 0 && !offsets) return ah_fail(c, AH_EINVALID, "%s: null buffer", what);
  return AH_OK;
}

// the error of a parse call: the last offending row and its kind for the caller, who quotes the row
int parse_result(ah_ctx* c, const char* func, int64_t* bad_row_host, int* bad_kind_host) {
  unsigned long long at = 0;
  const int rc = read_bad(c, &at);
  if (rc != AH_OK) return rc;
  if (at == 0) return AH_OK;
  const int64_t row = (int64_t)(at >> 2) - 1;
  const int kind = (int)(at & 3);
  if (bad_row_host) *bad_row_host = row;
  if (bad_kind_host) *bad_kind_host = kind;
  return ah_fail(c, AH_EINVALID, "strconv.%s: parsing row %lld: %s", func, (long long)row, kind == kScRange ? "value out of range" : "invalid syntax");
}

}  // namespace

AH_EXPORT int ah_parse_int(ah_ctx* c, int offset_width, const void* offsets, const uint8_t* data, const uint8_t* valid, int64_t off, int64_t n,
                           int out_type, void* out_values, int64_t* bad_row_host, int* bad_kind_host) {
  AH_ENTER(c);
  if (bad_row_host) *bad_row_host = -1;
  if (bad_kind_host) *bad_kind_host = 0;
  int rc = check_rows(c, "parse integer", offset_width, offsets, off, n);
  if (rc != AH_OK) return rc;
  int bytes = 0, is_signed = 0;
  if (!format_type(out_type, &bytes, &is_signed) || bytes == 0) return ah_fail(c, AH_EINVALID, "parse integer: type %d is not an integer", out_type);
  if (n == 0) return AH_OK;
  if (!out_values) return ah_fail(c, AH_EINVALID, "parse integer: null buffer");
  rc = arm_bad(c, 0);
  if (rc != AH_OK) return rc;
  const ByteRows rows = byte_rows(offset_width, offsets, data, 0, off);
  const unsigned grid = chunk_grid(c, n);
  uint8_t* out = (uint8_t*)out_values;
#define AH_PARSE(OW, B) parse_int_kernel<OW, B><<<grid, kBlock, 0, c->stream>>>(rows, valid, off, n, is_signed, out, bad_word(c))
  if (offset_width == 4) { if (bytes == 1) AH_PARSE(4, 1); else if (bytes == 2) AH_PARSE(4, 2); else if (bytes == 4) AH_PARSE(4, 4); else AH_PARSE(4, 8); }
  else { if (bytes == 1) AH_PARSE(8, 1); else if (bytes == 2) AH_PARSE(8, 2); else if (bytes == 4) AH_PARSE(8, 4); else AH_PARSE(8, 8); }
#undef AH_PARSE
  AH_LAUNCH_CHECK(c);
  return parse_result(c, is_signed ? "ParseInt" : "ParseUint", bad_row_host, bad_kind_host);
}

AH_EXPORT int ah_parse_bool(ah_ctx* c, int offset_width, const void* offsets, const uint8_t* data, const uint8_t* valid, int64_t off, int64_t n,
                            uint8_t* out_bits, int64_t* bad_row_host) {
  AH_ENTER(c);
  if (bad_row_host) *bad_row_host = -1;
  int rc = check_rows(c, "parse boolean", offset_width, offsets, off, n);
  if (rc != AH_OK) return rc;
  if (n == 0) return AH_OK;
  if (!out_bits) return ah_fail(c, AH_EINVALID, "parse boolean: null buffer");
  rc = arm_bad(c, 0);
  if (rc != AH_OK) return rc;
  const ByteRows rows = byte_rows(offset_width, offsets, data, 0, off);
  const unsigned grid = chunk_grid(c, n);
  const int aligned = ((uintptr_t)out_bits & 7) == 0;
  if (offset_width == 4) parse_bool_kernel<4><<<grid, kBlock, 0, c->stream>>>(rows, valid, off, n, out_bits, aligned, bad_word(c));
  else parse_bool_kernel<8><<<grid, kBlock, 0, c->stream>>>(rows, valid, off, n, out_bits, aligned, bad_word(c));
  AH_LAUNCH_CHECK(c);
  return parse_result(c, "ParseBool", bad_row_host, nullptr);
}

AH_EXPORT int ah_format_int_offsets(ah_ctx* c, int in_type, const void* values, const uint8_t* valid, int64_t off, int64_t n, int offset_width,
                                    void* out_offsets, int64_t* out_total_bytes_host) {
  AH_ENTER(c);
  if (out_total_bytes_host) *out_total_bytes_host = 0;
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "format: negative length/offset");
  if (offset_width != 4 && offset_width != 8) return ah_fail(c, AH_EINVALID, "format: binary offsets are 4 or 8 bytes wide");
  int bytes = 0, is_signed = 0;
  if (!format_type(in_type, &bytes, &is_signed)) return ah_fail(c, AH_EINVALID, "format: type %d is neither an integer nor boolean", in_type);
  if (!out_offsets || (n > 0 && !values)) return ah_fail(c, AH_EINVALID, "format: null buffer");
  if (n == 0) {  // a lone closing offset
    AH_HIP(c, hipMemsetAsync(out_offsets, 0, (size_t)offset_width, c->stream));
    return AH_OK;
  }
  VarOut v;
  int rc = varout_begin(c, n, 0, /*can_overflow=*/true, &v);
  if (rc != AH_OK) return rc;
  const unsigned grid = chunk_grid(c, n);
  const uint8_t* in = (const uint8_t*)values;
  switch (bytes) {
    case 0: format_lens_kernel<0><<<grid, kBlock, 0, c->stream>>>(in, valid, off, n, is_signed, v.lens); break;
    case 1: format_lens_kernel<1><<<grid, kBlock, 0, c->stream>>>(in, valid, off, n, is_signed, v.lens); break;
    case 2: format_lens_kernel<2><<<grid, kBlock, 0, c->stream>>>(in, valid, off, n, is_signed, v.lens); break;
    case 4: format_lens_kernel<4><<<grid, kBlock, 0, c->stream>>>(in, valid, off, n, is_signed, v.lens); break;
    default: format_lens_kernel<8><<<grid, kBlock, 0, c->stream>>>(in, valid, off, n, is_signed, v.lens); break;
  }
  AH_LAUNCH_CHECK(c);
  rc = varout_enqueue(c, v, n, offset_width, out_offsets, /*caller_words=*/false);
  if (rc != AH_OK) return rc;
  int64_t total = 0;
  bool over = false;
  rc = varout_finish(c, v, &total, &over);
  if (rc != AH_OK) return rc;
  if (over) return ah_fail(c, AH_EINVALID, "formatted cast: %lld bytes exceed the 32-bit offsets of the output", (long long)total);
  if (out_total_bytes_host) *out_total_bytes_host = total;
  return AH_OK;
}

AH_EXPORT int ah_format_int_data(ah_ctx* c, int in_type, const void* values, const uint8_t* valid, int64_t off, int64_t n, int offset_width,
                                 const void* out_offsets, uint8_t* out_data) {
  AH_ENTER(c);
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "format: negative length/offset");
  if (offset_width != 4 && offset_width != 8) return ah_fail(c, AH_EINVALID, "format: binary offsets are 4 or 8 bytes wide");
  int bytes = 0, is_signed = 0;
  if (!format_type(in_type, &bytes, &is_signed)) return ah_fail(c, AH_EINVALID, "format: type %d is neither an integer nor boolean", in_type);
  if (n == 0) return AH_OK;
  if (!values || !out_offsets || !out_data) return ah_fail(c, AH_EINVALID, "format: null buffer");
  const unsigned grid = ah_stream_grid(c, ah_ceil_div(n, kBlock), 8);
  const uint8_t* in = (const uint8_t*)values;
#define AH_FORMAT(B)                                                                                                                      \
  do {                                                                                                                                    \
    if (offset_width == 4) format_data_kernel<B, int32_t><<<grid, kBlock, 0, c->stream>>>(in, valid, off, n, is_signed, (const int32_t*)out_offsets, out_data); \
    else format_data_kernel<B, long long><<<grid, kBlock, 0, c->stream>>>(in, valid, off, n, is_signed, (const long long*)out_offsets, out_data);              \
  } while (0)
  switch (bytes) {
    case 0: AH_FORMAT(0); break;
    case 1: AH_FORMAT(1); break;
    case 2: AH_FORMAT(2); break;
    case 4: AH_FORMAT(4); break;
    default: AH_FORMAT(8); break;
  }
#undef AH_FORMAT
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

AH_EXPORT int ah_validate_utf8(ah_ctx* c, int offset_width, const void* offsets, const uint8_t* data, int byte_width, const uint8_t* valid,
                               int64_t off, int64_t n, int64_t* bad_row_host) {
  AH_ENTER(c);
  if (bad_row_host) *bad_row_host = -1;
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "validate UTF-8: negative length/offset");
  if (offset_width != 0 && offset_width != 4 && offset_width != 8) return ah_fail(c, AH_EINVALID, "validate UTF-8: offsets are 4 or 8 bytes wide, 0 for fixed-size rows");
  if (offset_width == 0 && byte_width < 0) return ah_fail(c, AH_EINVALID, "validate UTF-8: negative byte width");
  if (n == 0 || (offset_width == 0 && byte_width == 0)) return AH_OK;
  if ((offset_width != 0 && !offsets) || (offset_width == 0 && !data)) return ah_fail(c, AH_EINVALID, "validate UTF-8: null buffer");
  int rc = arm_bad(c, 0xFF);
  if (rc != AH_OK) return rc;
  const ByteRows rows = byte_rows(offset_width, offsets, data, byte_width, off);
  const unsigned grid = chunk_grid(c, n);
  if (offset_width == 4) validate_utf8_kernel<4><<<grid, kBlock, 0, c->stream>>>(rows, valid, off, n, bad_word(c));
  else if (offset_width == 8) validate_utf8_kernel<8><<<grid, kBlock, 0, c->stream>>>(rows, valid, off, n, bad_word(c));
  else validate_utf8_kernel<0><<<grid, kBlock, 0, c->stream>>>(rows, valid, off, n, bad_word(c));
  AH_LAUNCH_CHECK(c);
  unsigned long long at = ~0ull;
  rc = read_bad(c, &at);
  if (rc != AH_OK) return rc;
  if (at == ~0ull) return AH_OK;
  if (bad_row_host) *bad_row_host = (int64_t)at;
  return ah_fail(c, AH_EINVALID, "invalid UTF8 bytes in row %lld", (long long)at);
}

AH_EXPORT int ah_fixed_binary_offsets(ah_ctx* c, int offset_width, int byte_width, int64_t off, int64_t n, void* out_offsets) {
  AH_ENTER(c);
  if (n < 0 || off < 0 || byte_width < 0) return ah_fail(c, AH_EINVALID, "fixed-size binary offsets: negative length/offset/width");
  if (offset_width != 4 && offset_width != 8) return ah_fail(c, AH_EINVALID, "fixed-size binary offsets: 4 or 8 bytes wide");
  if (!out_offsets) return ah_fail(c, AH_EINVALID, "fixed-size binary offsets: null buffer");
  const int64_t last = (off + n) * (int64_t)byte_width;
  if (offset_width == 4 && last > 2147483647ll) return ah_fail(c, AH_EINVALID, "fixed-size binary offsets: %lld exceeds 32-bit offsets", (long long)last);
  const unsigned grid = ah_stream_grid(c, ah_ceil_div(n + 1, kBlock), 8);
  if (offset_width == 4) fixed_offsets_kernel<int32_t><<<grid, kBlock, 0, c->stream>>>(off, byte_width, n, (int32_t*)out_offsets);
  else fixed_offsets_kernel<long long><<<grid, kBlock, 0, c->stream>>>(off, byte_width, n, (long long*)out_offsets);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}
