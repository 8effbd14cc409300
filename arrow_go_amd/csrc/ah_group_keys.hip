// ah_group_keys.hip — ah_group_ids: the dense first-seen group ids of a TUPLE of key columns (String, fixed-size, Boolean, several of them).
//
// No reference analogue (arrow-go has no hash aggregate); definition in DESIGN.md §3.2.  Three ways to the ids:
//   one column      the call IS the matching encoder with nulls encoded: ah_hash.hip's 8-byte, byte-string or fixed-width path.
//   narrow tuples   every column fixed-width or Boolean, and (value bits) + (one bit per column with a validity buffer) ≤ 64:
//                   pack_kernel writes one 64-bit word per row — zeros under a null, the validity bit beside the value — and that
//                   column takes the 8-byte encoder with all of its routes (LDS tables, first look, partition-first).  Two rows
//                   are in one group iff their words are equal: a null row's word has its validity bit clear and nothing of its
//                   payload.  The all-ones word (possible only when 64 value bits are in use) is the tables' EMPTY marker, for
//                   which the encoder keeps a slot of its own.
//   everything else ah_hash.hip's global table with the TupleKeys policy: rows are hashed and compared where they lie.
// The packed column lives in the context's pack block (ah_pack_reserve, ah_common.h): the encode takes the scratch arena and, on the
// partition-first route, the temp arena, and a reservation that grows frees the old block.
//
// HBM of the pack pass: Σ column widths read + 8 B/row written, then the encoder's 8 B/row.
#include "ah_common.h"
#include "ah_hashing.h"
#include "ah_bytes.h"

namespace {

constexpr int kPackRows = 4;   // CONSECUTIVE rows per lane: a 4-byte column arrives as one 16-byte load, the words leave as two 16-byte stores
constexpr int kMaxKeys = 8;

struct PackCol {
  const uint8_t* data;    // the slot of row 0 of the call; Boolean: the bitmap (bit off + i)
  const uint8_t* valid;   // nullable; bit off + i
  int64_t off;
  int w;                  // bytes per slot (1 … 8); 0: Boolean
  int shift, vshift;      // where the value and — with a validity buffer — the validity bit go in the word
};
struct PackCols {
  PackCol col[kMaxKeys];
  int ncols;
};

// w bytes at p, little-endian, zero-extended (element alignment only: an Arrow slice)
__device__ __forceinline__ unsigned long long load_slot_bytes(const uint8_t* p, int w) {
  switch (w) {
    case 1: return *p;
    case 2: { unsigned short v; __builtin_memcpy(&v, p, 2); return v; }
    case 4: { unsigned v; __builtin_memcpy(&v, p, 4); return v; }
    case 8: return load8(p);
    default: return load_tail(p, w);
  }
}

// A wave holds 256 consecutive rows, lane l rows pos0 + 4·l … + 3: their bits of a bitmap (any bit offset) come as the wave's four
// 64-bit words through scalar loads (ah_wave_bits64), of which the lane keeps its nibble.  Rows past the column's end read as 0,
// a null bitmap as all ones — so the nibble of a validity bitmap is also "the row exists".
__device__ __forceinline__ unsigned lane_nibble(const uint8_t* __restrict__ bm, int64_t pos0, int64_t left, int lane) {
  unsigned long long mine = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const int64_t l = left - 64 * q;   // wave-uniform
    const unsigned long long wq = l > 0 ? ah_wave_bits64(bm, pos0 + 64 * q, l) : 0ull;
    if ((lane >> 4) == q) mine = wq;
  }
  return (unsigned)(mine >> ((lane & 15) * 4)) & 15u;
}

// One 64-bit word per row: zeros under a null, the validity bit beside the value.  The slots of a lane's four rows are one load of
// 4·w bytes for w = 1, 2, 4, 8 (neighbouring lanes read neighbouring bytes); other widths, and the lane that holds the column's end,
// go row by row.
__global__ __launch_bounds__(kBlock) void pack_kernel(const PackCols cols, int64_t n, unsigned long long* __restrict__ out) {
  const int lane = ah_lane();
  const int64_t stride = (int64_t)gridDim.x * kBlock * kPackRows;
  for (int64_t r0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * kPackRows; r0 - (int64_t)lane * kPackRows < n; r0 += stride) {
    const int64_t w0 = r0 - (int64_t)lane * kPackRows;   // the wave's first row: the loop bound is wave-uniform, lane_nibble sees all 64 lanes
    const bool whole = r0 + kPackRows <= n;
    unsigned long long word[kPackRows];
#pragma unroll
    for (int j = 0; j < kPackRows; j++) word[j] = 0;
#pragma unroll
    for (int c = 0; c < kMaxKeys; c++) {
      if (c >= cols.ncols) break;
      const PackCol& k = cols.col[c];
      const unsigned ok = lane_nibble(k.valid, k.off + w0, n - w0, lane);
      unsigned long long v[kPackRows];
#pragma unroll
      for (int j = 0; j < kPackRows; j++) v[j] = 0;
      if (k.w == 0) {
        const unsigned d = lane_nibble(k.data, k.off + w0, n - w0, lane);
#pragma unroll
        for (int j = 0; j < kPackRows; j++) v[j] = (d >> j) & 1u;
      } else if (whole && k.w == 4) {
        unsigned t[kPackRows];
        __builtin_memcpy(t, k.data + r0 * 4, sizeof(t));
#pragma unroll
        for (int j = 0; j < kPackRows; j++) v[j] = t[j];
      } else if (whole && k.w == 8) {
        __builtin_memcpy(v, k.data + r0 * 8, sizeof(v));
      } else if (whole && k.w == 2) {
        unsigned short t[kPackRows];
        __builtin_memcpy(t, k.data + r0 * 2, sizeof(t));
#pragma unroll
        for (int j = 0; j < kPackRows; j++) v[j] = t[j];
      } else if (whole && k.w == 1) {
        uint8_t t[kPackRows];
        __builtin_memcpy(t, k.data + r0, sizeof(t));
#pragma unroll
        for (int j = 0; j < kPackRows; j++) v[j] = t[j];
      } else {
#pragma unroll
        for (int j = 0; j < kPackRows; j++)
          if (r0 + j < n) v[j] = load_slot_bytes(k.data + (r0 + j) * (int64_t)k.w, k.w);
      }
#pragma unroll
      for (int j = 0; j < kPackRows; j++)
        if ((ok >> j) & 1u) word[j] |= (v[j] << k.shift) | (k.valid ? 1ull << k.vshift : 0ull);
    }
    if (whole) {
#pragma unroll
      for (int j = 0; j < kPackRows; j += 2) ah_st16<unsigned long long>(out + r0 + j, ah_vec16<unsigned long long>{{word[j], word[j + 1]}});
    } else {
#pragma unroll
      for (int j = 0; j < kPackRows; j++)
        if (r0 + j < n) out[r0 + j] = word[j];
    }
  }
}

int check_key(ah_ctx* c, const ah_group_key& k, int64_t n) {
  if (k.off < 0) return ah_fail(c, AH_EINVALID, "group_ids: negative length/offset");
  if (k.offset_width != 0 && k.offset_width != 4 && k.offset_width != 8) return ah_fail(c, AH_EINVALID, "group_ids: offset width must be 0, 4 or 8");
  if (k.bits != 0 && k.bits != 1) return ah_fail(c, AH_EINVALID, "group_ids: bits must be 0 or 1");
  if (k.bits && (k.byte_width != 0 || k.offset_width != 0)) return ah_fail(c, AH_EINVALID, "group_ids: a bits column has no byte width or offsets");
  if (k.offset_width && k.byte_width != 0) return ah_fail(c, AH_EINVALID, "group_ids: a column with offsets has no byte width");
  if (!k.offset_width && !k.bits && (k.byte_width < 1 || k.byte_width > 4096)) return ah_fail(c, AH_EINVALID, "group_ids: fixed width must be 1..4096 bytes");
  if (n == 0) return AH_OK;
  if (k.offset_width ? !k.offsets : !k.data) return ah_fail(c, AH_EINVALID, "group_ids: null buffer");
  if (k.offset_width && ((uintptr_t)k.offsets & (uintptr_t)(k.offset_width - 1))) return ah_fail(c, AH_EINVALID, "group_ids: offsets not element-aligned");
  return AH_OK;
}

}  // namespace

AH_EXPORT int ah_group_ids(ah_ctx* c, int nkeys, const ah_group_key* keys, int64_t n, int32_t* out_ids, int64_t* out_first_rows,
                           int64_t* out_ngroups_host) {
  AH_ENTER(c);
  if (nkeys < 1 || nkeys > kMaxKeys) return ah_fail(c, AH_EINVALID, "group_ids: 1 to 8 key columns");
  if (!keys) return ah_fail(c, AH_EINVALID, "group_ids: null key table");
  if (n < 0) return ah_fail(c, AH_EINVALID, "group_ids: negative length/offset");
  for (int j = 0; j < nkeys; j++)
    if (int rc = check_key(c, keys[j], n)) return rc;
  if (out_ngroups_host) *out_ngroups_host = 0;
  if (n == 0) return AH_OK;
  if (!out_ids || !out_first_rows) return ah_fail(c, AH_EINVALID, "group_ids: null buffer");
  if (n > ((int64_t)1 << 30)) return ah_fail(c, AH_ENOTIMPL, "group_ids: more than 2^30 rows per call");
  int64_t ngroups = 0;
  int rc;
  const ah_group_key& k0 = keys[0];
  if (nkeys == 1 && k0.offset_width) {
    rc = ah_hash_binary_encode(c, k0.offset_width, k0.offsets, k0.data, k0.valid, k0.off, n, 1, out_ids, nullptr, out_first_rows, &ngroups, nullptr);
  } else if (nkeys == 1 && k0.byte_width == 8 && ((uintptr_t)k0.data & 7) == 0) {
    rc = ah_encode_u64_first_seen(c, (const uint64_t*)k0.data + k0.off, k0.valid, k0.off, n, out_ids, out_first_rows, &ngroups);
  } else if (nkeys == 1 && !k0.bits) {
    rc = ah_hash_fixed_encode(c, k0.byte_width, k0.data, k0.valid, k0.off, n, 1, out_ids, nullptr, out_first_rows, nullptr, &ngroups, nullptr);
  } else {
    // the bit budget of the packed word: value bits, and one bit per column that has a validity buffer
    int bits = 0;
    bool narrow = true;
    PackCols pc;
    pc.ncols = nkeys;
    for (int j = 0; j < kMaxKeys; j++) pc.col[j] = PackCol{nullptr, nullptr, 0, 0, 0, 0};
    for (int j = 0; j < nkeys && narrow; j++) {
      const ah_group_key& k = keys[j];
      if (k.offset_width || (!k.bits && k.byte_width > 8)) { narrow = false; break; }
      const int vb = k.bits ? 1 : 8 * k.byte_width;
      if (bits + vb + (k.valid ? 1 : 0) > 64) { narrow = false; break; }
      pc.col[j] = PackCol{k.bits ? k.data : k.data + k.off * (int64_t)k.byte_width, k.valid, k.off, k.bits ? 0 : k.byte_width, bits, k.valid ? bits + vb : 0};
      bits += vb + (k.valid ? 1 : 0);
    }
    if (narrow) {
      void* packed = nullptr;
      if ((rc = ah_pack_reserve(c, (size_t)n * 8, &packed)) != AH_OK) return rc;
      pack_kernel<<<ah_stream_grid(c, ah_ceil_div(n, (int64_t)kBlock * kPackRows), /*default_bpc=*/0), kBlock, 0, c->stream>>>(pc, n, (unsigned long long*)packed);
      AH_LAUNCH_CHECK(c);
      rc = ah_encode_u64_first_seen(c, (const uint64_t*)packed, nullptr, 0, n, out_ids, out_first_rows, &ngroups);
    } else {
      rc = ah_encode_tuple_first_seen(c, nkeys, keys, n, out_ids, out_first_rows, &ngroups);
    }
  }
  if (rc != AH_OK) return rc;
  AH_HIP(c, hipStreamSynchronize(c->stream));
  if (out_ngroups_host) *out_ngroups_host = ngroups;
  return AH_OK;
}
