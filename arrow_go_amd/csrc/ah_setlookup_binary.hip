// ah_setlookup_binary.hip — is_in of byte-string keys: String / Binary / LargeString / LargeBinary, FixedSizeBinary of any
// width, Decimal128 / Decimal256 (row §8(f)-2), and the index gather of a dictionary input.
//
// Replaces SetLookupState[[]byte].Init + visitBinary + isInKernelExec (arrow/compute/internal/kernels/scalar_set_lookup.go:
// 192-244, 270-300, 374-413) behind compute's "is_in" (compute/scalar_set_lookup.go:207-232).  Values compare as bytes: a
// base-binary value by its offsets range (so "" is a value), a fixed-width value by its byte_width raw bytes.  The
// null-behaviour truth table is ah_setlookup.h's, shared with the 1/2/4/8-byte kernels.
//
// The set becomes an open-addressing table of 64-bit slot words {tag = hash bits 63..32 | set row}, load ≤ ¼, linear
// probing — the binary memo table of ah_hash.hip.  A set row's bytes are reached through a side table of (pointer, length)
// written per value-set piece before the table is built, so a chunked value set goes into ONE table without being
// concatenated.  Set nulls are a flag.  Tiers: ≤ 1024 values → 32 KiB of LDS per 256-thread workgroup;
// ≤ 4096 values → 128 KiB of LDS, one 1024-thread workgroup per CU; larger sets probe the table in HBM.
//
// Probe: one 64-row chunk per wave step, one row per lane: read offsets i and i + 1, hash the bytes, walk the table
// comparing tags, and compare bytes only on a tag hit.  The result is one ballot per 64 rows, stored as a whole 64-bit
// word (read-modify-write only where the output range is not word-aligned).
// Long values: a lane hashes at most the first kHashPrefix bytes (plus the length and the last 8 bytes) and compares at
// most kLaneCmp bytes itself.  A tag hit on a longer value is handed to the whole wave, which compares it 512 bytes per
// step (64 lanes × 8 bytes), one pending row after another (wave_compare of ah_bytes.h, shared with the comparisons).  So
// no lane walks more than kHashPrefix + kLaneCmp bytes on its own, whatever the longest value of its wave.  Rows are read
// through ah_bytes.h's ByteRows; result words are stored by put_word (ah_common.h).
#include <vector>

#include "ah_common.h"
#include "ah_bytes.h"
#include "ah_setlookup.h"

namespace {

constexpr int kBlock = 256;
constexpr int kLdsSlots = 4096;       // 32 KiB: sets of up to 1024 values
constexpr int kLdsSlotsBig = 16384;   // 128 KiB of gfx950's 160 KiB: sets of up to 4096 values, one workgroup per CU
constexpr int kBlockBig = 1024;
constexpr unsigned long long kEmpty = ~0ull;
constexpr int64_t kHashPrefix = 256;  // bytes a lane hashes at most
constexpr int64_t kLaneCmp = 64;      // bytes a lane compares at most; longer values are compared by the wave

// the table's hash: hash_bytes (ah_bytes.h, shared with unique / dictionary_encode) of the value, or for a value longer than
// kHashPrefix of its first kHashPrefix bytes mixed with its length and last 8 bytes.  Membership needs SOME hash that equal
// byte strings share; this one bounds a lane's work.
__device__ __forceinline__ uint64_t key_hash(const uint8_t* p, int64_t len) {
  if (len <= kHashPrefix) return hash_bytes(p, len);
  uint64_t h = hash_bytes(p, kHashPrefix) ^ ((uint64_t)len * 0xC2B2AE3D27D4EB4Full);
  h = (h ^ load8(p + len - 8)) * 0xFF51AFD7ED558CCDull;
  return h ^ (h >> 32);
}

// ---- build -------------------------------------------------------------------------------------------------------------
// side table entries [base, base + n) for one piece: (pointer, length) of each value, length −1 for a null
template <int OW>
__global__ __launch_bounds__(kBlock) void set_refs_kernel(ByteRows rows, const uint8_t* __restrict__ valid, int64_t off, int64_t n, int64_t base,
                                                          unsigned long long* __restrict__ ref_ptr, long long* __restrict__ ref_len,
                                                          unsigned* __restrict__ flags) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    if (valid && !ah_bit(valid, off + i)) {
      atomicOr(flags, kFlagSetHasNull);
      ref_ptr[base + i] = 0;
      ref_len[base + i] = -1;
      continue;
    }
    const uint8_t* p;
    int64_t len;
    row_at<OW>(rows, i, &p, &len);
    ref_ptr[base + i] = (unsigned long long)(uintptr_t)p;
    ref_len[base + i] = len;
  }
}

// every non-null set row into the table; duplicates keep the first slot that holds their bytes.  The side table was
// written by earlier launches, so the row behind any slot word is readable here.
__global__ __launch_bounds__(kBlock) void set_insert_kernel(const unsigned long long* __restrict__ ref_ptr, const long long* __restrict__ ref_len,
                                                            int64_t n, unsigned long long* __restrict__ table, unsigned mask) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < n; r += stride) {
    const int64_t len = ref_len[r];
    if (len < 0) continue;
    const uint8_t* p = (const uint8_t*)(uintptr_t)ref_ptr[r];
    const uint64_t h = key_hash(p, len);
    const unsigned long long word = (h & 0xFFFFFFFF00000000ull) | (unsigned long long)(unsigned)r;  // never all-ones: r < 2^31
    unsigned idx = (unsigned)h & mask;
    for (;;) {  // load ≤ ¼: always terminates
      const unsigned long long prev = atomicCAS(&table[idx], kEmpty, word);
      if (prev == kEmpty) break;
      if ((prev >> 32) == (word >> 32)) {
        const unsigned pr = (unsigned)prev;
        if (ref_len[pr] == len && equal_bytes(p, (const uint8_t*)(uintptr_t)ref_ptr[pr], len)) break;
      }
      idx = (idx + 1) & mask;
    }
  }
}

// ---- probe -------------------------------------------------------------------------------------------------------------
// MODE 1: table in LDS (≤ kLdsSlots) · 2: table in HBM · 3: table in LDS, kLdsSlotsBig slots, 1024-thread workgroups
template <int OW, int MODE, bool HAS_VALID, int BLOCK = (MODE == 3 ? kBlockBig : kBlock)>
__global__ __launch_bounds__(BLOCK) void is_in_bytes_kernel(ByteRows rows, const uint8_t* __restrict__ valid, int64_t off, int64_t n,
                                                            const unsigned long long* __restrict__ table, unsigned mask,
                                                            const unsigned long long* __restrict__ ref_ptr, const long long* __restrict__ ref_len,
                                                            const unsigned* __restrict__ flags, int null_behavior, int aligned,
                                                            uint8_t* __restrict__ out_data, uint8_t* __restrict__ out_valid, int64_t out_off) {
  __shared__ unsigned long long s_tab[MODE == 1 ? kLdsSlots : (MODE == 3 ? kLdsSlotsBig : 1)];
  if (MODE != 2) {
    for (unsigned i = threadIdx.x; i <= mask; i += BLOCK) s_tab[i] = table[i];
    __syncthreads();
  }
  const NullRule rule = null_rule(flags[0], null_behavior);
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (BLOCK / 64);
  for (int64_t ch = (int64_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const int cnt = left >= 64 ? 64 : (int)left;
    const unsigned long long range = cnt == 64 ? ~0ull : ((1ull << cnt) - 1ull);
    const unsigned long long in_valid = HAS_VALID ? ah_load_bits64(valid, off + ch * 64, cnt) : range;
    bool pend = (in_valid >> lane) & 1ull, found = false, coop = false;
    const uint8_t* p = nullptr;
    const uint8_t* q = nullptr;
    int64_t len = 0;
    unsigned idx = 0, tag = 0;
    if (pend) {
      row_at<OW>(rows, row, &p, &len);
      const uint64_t h = key_hash(p, len);
      idx = (unsigned)h & mask;
      tag = (unsigned)(h >> 32);
    }
    for (;;) {
      // lane-local probing until this lane is done or holds a tag hit on a long value
      while (pend && !coop) {
        const unsigned long long sl = MODE == 2 ? table[idx] : s_tab[idx];
        if (sl == kEmpty) { pend = false; break; }
        if ((unsigned)(sl >> 32) == tag) {
          const unsigned r = (unsigned)sl;
          const int64_t ql = OW == 0 ? len : (int64_t)ref_len[r];
          if (ql == len) {
            q = (const uint8_t*)(uintptr_t)ref_ptr[r];
            if (len > kLaneCmp) { coop = true; break; }
            if (equal_bytes(p, q, len)) { found = true; pend = false; break; }
          }
        }
        idx = (idx + 1) & mask;
      }
      unsigned long long need = __ballot(coop);
      if (!need) break;  // every lane is done
      wave_compare<false>(need, p, q, len, 0, [&](int diff) {  // the wave compares each pending long value
        coop = false;
        if (!diff) { found = true; pend = false; }
        else idx = (idx + 1) & mask;
      });
    }
    const unsigned long long fw = __ballot(found);
    const unsigned long long nulls = ~in_valid & range;
    const unsigned long long dword = fw | (rule.dnull ? nulls : 0ull);
    const unsigned long long vword = fw | (rule.vmiss ? in_valid : 0ull) | (rule.vnull ? nulls : 0ull);
    if (lane == 0) {
      put_word(out_data, out_off, aligned, ch, dword, cnt);
      put_word(out_valid, out_off, aligned, ch, vword, cnt);
    }
  }
}

template <int OW, int MODE>
void launch_bytes_probe(ah_ctx* c, unsigned grid, const ByteRows& rows, const uint8_t* valid, int64_t off, int64_t n,
                        const unsigned long long* table, unsigned mask, const unsigned long long* ref_ptr, const long long* ref_len,
                        const unsigned* flags, int nb, uint8_t* out_data, uint8_t* out_valid, int64_t out_off) {
  const int aligned = (out_off & 63) == 0 && (((uintptr_t)out_data | (uintptr_t)out_valid) & 7) == 0;
  constexpr int block = MODE == 3 ? kBlockBig : kBlock;
  if (valid)
    is_in_bytes_kernel<OW, MODE, true><<<grid, block, 0, c->stream>>>(rows, valid, off, n, table, mask, ref_ptr, ref_len, flags, nb, aligned,
                                                                     out_data, out_valid, out_off);
  else
    is_in_bytes_kernel<OW, MODE, false><<<grid, block, 0, c->stream>>>(rows, valid, off, n, table, mask, ref_ptr, ref_len, flags, nb, aligned,
                                                                      out_data, out_valid, out_off);
}

template <int OW>
int run_bytes_probe(ah_ctx* c, const void* offsets, const uint8_t* data, int w, const uint8_t* valid, int64_t off, int64_t n, int nset,
                    const ah_set_chunk* set, int nb, uint8_t* out_data, uint8_t* out_valid, int64_t out_off) {
  const ByteRows rows = byte_rows(OW, offsets, data, w, off);
  int64_t set_n = 0;
  for (int i = 0; i < nset; i++) set_n += set[i].n;
  unsigned long long cap = 64;  // load ≤ ¼
  while (cap < 4ull * (unsigned long long)set_n) cap <<= 1;
  if (cap > (1ull << 31)) return ah_fail(c, AH_ENOTIMPL, "is_in: value set too large (%lld)", (long long)set_n);
  // scratch: flags (128 B) | table (cap · 8) | side table: pointers (set_n · 8), lengths (set_n · 8)
  const size_t table_bytes = (size_t)cap * 8, ref_bytes = (size_t)(set_n > 0 ? set_n : 1) * 8;
  void* scratch;
  int rc = ah_scratch_reserve(c, 128 + table_bytes + 2 * ref_bytes, &scratch);
  if (rc != AH_OK) return rc;
  unsigned* flags = (unsigned*)scratch;
  unsigned long long* table = (unsigned long long*)((uint8_t*)scratch + 128);
  unsigned long long* ref_ptr = (unsigned long long*)((uint8_t*)table + table_bytes);
  long long* ref_len = (long long*)((uint8_t*)ref_ptr + ref_bytes);
  AH_HIP(c, hipMemsetAsync(flags, 0, 128, c->stream));
  AH_HIP(c, hipMemsetAsync(table, 0xFF, table_bytes, c->stream));
  int64_t base = 0;
  for (int i = 0; i < nset; i++) {
    const ah_set_chunk& sc = set[i];
    if (sc.n == 0) continue;
    const unsigned g = ah_stream_grid(c, ah_ceil_div(sc.n, kBlock), 8);
    const ByteRows piece = byte_rows(sc.offset_width, sc.offsets, sc.data, w, sc.off);
    if (sc.offset_width == 4) set_refs_kernel<4><<<g, kBlock, 0, c->stream>>>(piece, sc.valid, sc.off, sc.n, base, ref_ptr, ref_len, flags);
    else if (sc.offset_width == 8) set_refs_kernel<8><<<g, kBlock, 0, c->stream>>>(piece, sc.valid, sc.off, sc.n, base, ref_ptr, ref_len, flags);
    else set_refs_kernel<0><<<g, kBlock, 0, c->stream>>>(piece, sc.valid, sc.off, sc.n, base, ref_ptr, ref_len, flags);
    AH_LAUNCH_CHECK(c);
    base += sc.n;
  }
  if (set_n > 0) {
    set_insert_kernel<<<ah_stream_grid(c, ah_ceil_div(set_n, kBlock), 8), kBlock, 0, c->stream>>>(ref_ptr, ref_len, set_n, table, (unsigned)(cap - 1));
    AH_LAUNCH_CHECK(c);
  }
  const int64_t nchunks = ah_ceil_div(n, 64);
  const unsigned mask = (unsigned)(cap - 1);
  if (cap <= (unsigned long long)kLdsSlots) {
    const unsigned grid = ah_stream_grid(c, ah_ceil_div(nchunks, kBlock / 64), 8);
    launch_bytes_probe<OW, 1>(c, grid, rows, valid, off, n, table, mask, ref_ptr, ref_len, flags, nb, out_data, out_valid, out_off);
  } else if (cap <= (unsigned long long)kLdsSlotsBig) {
    const unsigned need = (unsigned)ah_ceil_div(nchunks, kBlockBig / 64), per_cu = (unsigned)c->num_cu;
    launch_bytes_probe<OW, 3>(c, need < per_cu ? need : per_cu, rows, valid, off, n, table, mask, ref_ptr, ref_len, flags, nb, out_data, out_valid,
                              out_off);
  } else {
    const unsigned grid = ah_stream_grid(c, ah_ceil_div(nchunks, kBlock / 64), 8);
    launch_bytes_probe<OW, 2>(c, grid, rows, valid, off, n, table, mask, ref_ptr, ref_len, flags, nb, out_data, out_valid, out_off);
  }
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

int check_common(ah_ctx* c, int64_t off, int64_t n, int nset, const ah_set_chunk* set, int nb, uint8_t* out_data, uint8_t* out_valid,
                 int64_t out_off) {
  if (n < 0 || off < 0 || out_off < 0 || nset < 0) return ah_fail(c, AH_EINVALID, "is_in: negative length/offset");
  if (nb < AH_NULL_MATCH || nb > AH_NULL_INCONCLUSIVE) return ah_fail(c, AH_EINVALID, "is_in: bad null matching behavior %d", nb);
  if (nset > 0 && !set) return ah_fail(c, AH_EINVALID, "is_in: null value-set table");
  for (int i = 0; i < nset; i++)
    if (set[i].n < 0 || set[i].off < 0) return ah_fail(c, AH_EINVALID, "is_in: negative value-set piece length/offset");
  if (n > 0 && (!out_data || !out_valid)) return ah_fail(c, AH_EINVALID, "is_in: null buffer");
  return AH_OK;
}

// ---- dictionary inputs: bit indices[i] of the dictionary's results ----------------------------------------------------------
template <typename IdxT, bool HAS_VALID>
__global__ __launch_bounds__(kBlock) void dict_gather_kernel(const IdxT* __restrict__ indices, const uint8_t* __restrict__ valid, int64_t off,
                                                             int64_t n, const uint8_t* __restrict__ lut_data, const uint8_t* __restrict__ lut_valid,
                                                             int64_t lut_n, int aligned, uint8_t* __restrict__ out_data,
                                                             uint8_t* __restrict__ out_valid, int64_t out_off) {
  const int lane = threadIdx.x & 63;
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t row = ch * 64 + lane;
    const int64_t left = n - ch * 64;
    const int cnt = left >= 64 ? 64 : (int)left;
    bool d = false, v = false;
    if (lane < cnt) {
      const bool ok = HAS_VALID ? ah_bit(valid, off + row) : true;
      const long long k = ok ? (long long)indices[off + row] : (long long)lut_n;  // a null index: the result of a null value
      if (k >= 0 && k <= lut_n) {
        d = ah_bit(lut_data, k);
        v = ah_bit(lut_valid, k);
      }
    }
    const unsigned long long dword = __ballot(d), vword = __ballot(v);
    if (lane == 0) {
      put_word(out_data, out_off, aligned, ch, dword, cnt);
      put_word(out_valid, out_off, aligned, ch, vword, cnt);
    }
  }
}

template <typename IdxT>
void launch_gather(ah_ctx* c, const void* indices, const uint8_t* valid, int64_t off, int64_t n, const uint8_t* lut_data, const uint8_t* lut_valid,
                   int64_t lut_n, uint8_t* out_data, uint8_t* out_valid, int64_t out_off) {
  const int aligned = (out_off & 63) == 0 && (((uintptr_t)out_data | (uintptr_t)out_valid) & 7) == 0;
  const unsigned grid = ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, 64), kBlock / 64), 8);
  if (valid)
    dict_gather_kernel<IdxT, true><<<grid, kBlock, 0, c->stream>>>((const IdxT*)indices, valid, off, n, lut_data, lut_valid, lut_n, aligned, out_data,
                                                                  out_valid, out_off);
  else
    dict_gather_kernel<IdxT, false><<<grid, kBlock, 0, c->stream>>>((const IdxT*)indices, valid, off, n, lut_data, lut_valid, lut_n, aligned, out_data,
                                                                   out_valid, out_off);
}

}  // namespace

AH_EXPORT int ah_is_in_binary(ah_ctx* c, int offset_width, const void* offsets, const uint8_t* data, const uint8_t* valid, int64_t off, int64_t n,
                              int set_nchunks, const ah_set_chunk* set, int null_behavior, uint8_t* out_data, uint8_t* out_valid,
                              int64_t out_bit_offset) {
  AH_ENTER(c);
  int rc = check_common(c, off, n, set_nchunks, set, null_behavior, out_data, out_valid, out_bit_offset);
  if (rc != AH_OK) return rc;
  if (offset_width != 4 && offset_width != 8) return ah_fail(c, AH_EINVALID, "is_in: offset width must be 4 or 8 (got %d)", offset_width);
  for (int i = 0; i < set_nchunks; i++)
    if (set[i].offset_width != 4 && set[i].offset_width != 8)
      return ah_fail(c, AH_EINVALID, "is_in: value-set piece %d is not base-binary (offset width %d)", i, set[i].offset_width);
    else if (set[i].n > 0 && !set[i].offsets)
      return ah_fail(c, AH_EINVALID, "is_in: value-set piece %d has no offsets", i);
  if (n == 0) return AH_OK;
  if (!offsets) return ah_fail(c, AH_EINVALID, "is_in: null offsets");
  if (offset_width == 4) return run_bytes_probe<4>(c, offsets, data, 0, valid, off, n, set_nchunks, set, null_behavior, out_data, out_valid, out_bit_offset);
  return run_bytes_probe<8>(c, offsets, data, 0, valid, off, n, set_nchunks, set, null_behavior, out_data, out_valid, out_bit_offset);
}

AH_EXPORT int ah_is_in_fixed(ah_ctx* c, int byte_width, const uint8_t* data, const uint8_t* valid, int64_t off, int64_t n, int set_nchunks,
                             const ah_set_chunk* set, int null_behavior, uint8_t* out_data, uint8_t* out_valid, int64_t out_bit_offset) {
  AH_ENTER(c);
  int rc = check_common(c, off, n, set_nchunks, set, null_behavior, out_data, out_valid, out_bit_offset);
  if (rc != AH_OK) return rc;
  if (byte_width <= 0) return ah_fail(c, AH_EINVALID, "is_in: byte width must be positive (got %d)", byte_width);
  for (int i = 0; i < set_nchunks; i++)
    if (set[i].offset_width != 0) return ah_fail(c, AH_EINVALID, "is_in: value-set piece %d is not fixed-width", i);
    else if (set[i].n > 0 && !set[i].data) return ah_fail(c, AH_EINVALID, "is_in: value-set piece %d has no data", i);
  if (n == 0) return AH_OK;
  if (!data) return ah_fail(c, AH_EINVALID, "is_in: null buffer");
  if (byte_width == 1 || byte_width == 2 || byte_width == 4 || byte_width == 8) {  // SetLookupState[uintN] (kernels/scalar_set_lookup.go:106-133)
    SetPart parts[64];
    std::vector<SetPart> many;
    SetPart* pp = parts;
    if (set_nchunks > 64) { many.resize(set_nchunks); pp = many.data(); }
    for (int i = 0; i < set_nchunks; i++) pp[i] = SetPart{set[i].data + set[i].off * byte_width, set[i].valid, set[i].off, set[i].n};
    return ah_is_in_parts(c, byte_width, data + off * byte_width, valid, off, n, set_nchunks, pp, null_behavior, out_data, out_valid, out_bit_offset);
  }
  return run_bytes_probe<0>(c, nullptr, data, byte_width, valid, off, n, set_nchunks, set, null_behavior, out_data, out_valid, out_bit_offset);
}

AH_EXPORT int ah_is_in_dict_gather(ah_ctx* c, int index_width, const void* indices, const uint8_t* valid, int64_t off, int64_t n,
                                   const uint8_t* lut_data, const uint8_t* lut_valid, int64_t lut_n, uint8_t* out_data, uint8_t* out_valid,
                                   int64_t out_bit_offset) {
  AH_ENTER(c);
  if (n < 0 || off < 0 || lut_n < 0 || out_bit_offset < 0) return ah_fail(c, AH_EINVALID, "is_in: negative length/offset");
  if (n == 0) return AH_OK;
  if (!indices || !lut_data || !lut_valid || !out_data || !out_valid) return ah_fail(c, AH_EINVALID, "is_in: null buffer");
  switch (index_width) {
    case 1: launch_gather<int8_t>(c, indices, valid, off, n, lut_data, lut_valid, lut_n, out_data, out_valid, out_bit_offset); break;
    case 2: launch_gather<int16_t>(c, indices, valid, off, n, lut_data, lut_valid, lut_n, out_data, out_valid, out_bit_offset); break;
    case 4: launch_gather<int32_t>(c, indices, valid, off, n, lut_data, lut_valid, lut_n, out_data, out_valid, out_bit_offset); break;
    case 8: launch_gather<long long>(c, indices, valid, off, n, lut_data, lut_valid, lut_n, out_data, out_valid, out_bit_offset); break;
    default: return ah_fail(c, AH_EINVALID, "is_in: dictionary index width must be 1, 2, 4 or 8 (got %d)", index_width);
  }
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}
