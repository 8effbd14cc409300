// ah_sort.hip — sort_indices of one numeric array: stable LSD radix sort (row §8(f)-2).
//
// Replaces kernels.SortIndices for a single key over one array (arrow/compute/internal/kernels/
// vector_sort.go:388-481 → arraySortOneColumnRange, vector_sort_internal.go:252-273) behind
// compute's "sort_indices" (compute/vector_sort.go:42-52):
//   stable; nulls partitioned to the end or the start (key.NullPlacement), NaNs next to them
//   ([rest, NaNs, nulls] / [nulls, NaNs, rest] — partitionNullLikes :90-140: NaN placement follows the
//   null placement, not the order), the rest ordered by cmp.Compare, negated for Descending
//   (vector_sort_support.go:88-94): ties keep their input order in BOTH directions, −0.0 == +0.0.
// The reference is partition + slices.SortStableFunc with a comparator closure per pair.
//
// Here: (1) one stable 3-way partition pass straight off the column (category = rest / NaN / null)
// that also maps every value to an order-preserving unsigned key (sign flip for ints, the IEEE trick
// for floats with −0 → +0, complemented for Descending) and pairs it with its 32-bit row number;
// (2) a bitwise AND / OR reduction of the keys tells which key bytes vary at all; (3) one stable
// 8-bit LSD pass per varying byte over the `rest` range only — per pass: tile histograms →
// exclusive scan → scatter, the in-tile ranks from wave-level match-any (8 ballots) so the pass is
// stable by construction; (4) widening the row numbers to the uint64 output.  Equal keys never
// change relative order in any pass, which is exactly SortStableFunc's contract, and the NaN / null
// groups keep their input order because only pass (1) ever moves them.
// Traffic: 8 (+1/8) B/row for (1) and (2), ≈ 32 B/row per LSD pass ((key, row) read twice, written
// once), 12 B/row for (4): an Int64 column with all 8 bytes varying moves ≈ 290 B/row.
#include <algorithm>
#include <type_traits>
#include <vector>
#include "ah_sort_radix.h"

namespace {

// ---- the element source of a pass -------------------------------------------------------------
// Column<T>: pass (1) — reads the column, digit = category, emits (key, row).
// Pairs:     an LSD pass — reads (key, row) pairs, digit = a key byte.
template <typename T>
struct Column {
  const T* values;
  const uint8_t* valid;
  int64_t off;
  int descending, nulls_at_start;
  const unsigned* rows_in;  // the order produced by the less significant sort keys; NULL = input order
  __device__ __forceinline__ void load(int64_t i, unsigned long long* key, unsigned* row, unsigned* digit) const {
    const unsigned r = rows_in ? rows_in[i] : (unsigned)i;
    const T v = values[r];
    int cat = kCatRest;
    if (!ah_bit(valid, off + r)) cat = kCatNull;
    else if (std::is_floating_point<T>::value && v != v) cat = kCatNaN;
    *key = cat == kCatRest ? make_key<T>(v, descending) : 0ull;
    *row = r;
    *digit = nulls_at_start ? (unsigned)(2 - cat) : (unsigned)cat;  // [nulls, NaNs, rest] or [rest, NaNs, nulls]
  }
};
// group-by helper: (value bits, group id) pairs, digit = a byte of the group id
struct IdVal {
  const int32_t* ids;
  const unsigned long long* vals;
  const uint8_t* vvalid;
  int64_t voff;
  int shift;
  __device__ __forceinline__ void load(int64_t i, unsigned long long* key, unsigned* row, unsigned* digit) const {
    const unsigned g = (unsigned)ids[i];
    const bool ok = ah_bit(vvalid, voff + i);
    *key = ok ? vals[i] : 0ull;
    *row = ok ? g : (g | 0x80000000u);
    *digit = (g >> shift) & 255u;
  }
};

// second pass of the group-by partition: pairs already carry the null flag in bit 31 of the id
struct ValId {
  const unsigned long long* vals;
  const unsigned* ids;
  int shift;
  __device__ __forceinline__ void load(int64_t i, unsigned long long* key, unsigned* row, unsigned* digit) const {
    *key = vals[i];
    *row = ids[i];
    *digit = ((*row & 0x7fffffffu) >> shift) & 255u;
  }
};

// Pass (1) without the partition, for a column with no validity bitmap in input order: keys and row numbers in one streaming
// pass, the AND / OR / min / max of the keys on the way (per workgroup: res[5 b …] = {AND, OR, min, max, NaN count}).  Valid
// only if the NaN count comes back zero — then every row is `rest` and pass (2) has been done too; otherwise the caller
// runs the partition pass as usual.
template <typename T>
__global__ __launch_bounds__(kBlock) void pairs_kernel(const T* __restrict__ values, int64_t n, int descending, unsigned long long* __restrict__ keys,
                                                        unsigned* __restrict__ rows, unsigned long long* __restrict__ res) {
  KeyStats st;
  st.init();
  constexpr int U = 4;
  const int64_t stride = (int64_t)gridDim.x * kBlock * U;
  for (int64_t base = (int64_t)blockIdx.x * kBlock * U + threadIdx.x; base < n; base += stride) {
    T v[U];
#pragma unroll
    for (int u = 0; u < U; u++) { const int64_t i = base + (int64_t)u * kBlock; v[u] = i < n ? __builtin_nontemporal_load(&values[i]) : (T)0; }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = base + (int64_t)u * kBlock;
      if (i >= n) continue;
      if (std::is_floating_point<T>::value && v[u] != v[u]) { st.nans++; continue; }
      const unsigned long long k = make_key<T>(v[u], descending);
      __builtin_nontemporal_store(k, &keys[i]);
      __builtin_nontemporal_store((unsigned)i, &rows[i]);
      st.add(k);
    }
  }
  st = ah_block_reduce<kBlock>(st);
  if (threadIdx.x == 0) st.store<5>(res + (size_t)blockIdx.x * 5);
}

__global__ __launch_bounds__(kBlock) void emit_kernel(const unsigned* __restrict__ rows, int64_t n, uint64_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = rows[i];
}


// Stable sort of the current row order (rows_in, or the input order) by ONE column.  Leaves the new
// order in b.ra; returns through *result which buffer holds it (always b.ra).
template <typename T>
int sort_by_column(ah_ctx* c, SortBuffers& b, const void* values, const uint8_t* valid, int64_t off, int64_t n, int descending,
                   int nulls_at_start, const unsigned* rows_in) {
  const int64_t ntiles = ah_ceil_div(n, (int64_t)kTile * tiles_per_block(n));  // histogram rows ("blocks")
  int rc;
  // (1) partition by category, keys and row numbers come into being
  Column<T> col{(const T*)values, valid, off, descending, nulls_at_start, rows_in};
  int64_t rest_lo = 0, rest_n = 0;
  unsigned long long k_and = ~0ull, k_or = 0, kmin = ~0ull, kmax = 0;
  bool have_stats = false;
  if (valid == nullptr && rows_in == nullptr && n >= ((int64_t)1 << 20)) {
    // no validity bitmap, input order: nothing to partition unless a float column holds NaNs — one streaming pass, checked after
    // b.andor holds kAndOrGrid × 8 words (sort_buffers): the grid is clamped to that whatever ARROWHIP_BLOCKS_PER_CU asks for
    const unsigned pgrid = std::min(ah_stream_grid(c, ah_ceil_div(n, (int64_t)kBlock * 4), 8), (unsigned)kAndOrGrid);
    pairs_kernel<T><<<pgrid, kBlock, 0, c->stream>>>((const T*)values, n, descending, b.ka, b.ra, b.andor);
    AH_LAUNCH_CHECK(c);
    std::vector<unsigned long long> parts((size_t)pgrid * 5);
    AH_HIP(c, hipMemcpyAsync(parts.data(), b.andor, parts.size() * 8, hipMemcpyDeviceToHost, c->stream));
    AH_HIP(c, hipStreamSynchronize(c->stream));
    unsigned long long nans = 0;
    for (unsigned g = 0; g < pgrid; g++) {
      k_and &= parts[g * 5]; k_or |= parts[g * 5 + 1];
      kmin = parts[g * 5 + 2] < kmin ? parts[g * 5 + 2] : kmin;
      kmax = parts[g * 5 + 3] > kmax ? parts[g * 5 + 3] : kmax;
      nans += parts[g * 5 + 4];
    }
    if (nans == 0) { have_stats = true; rest_lo = 0; rest_n = n; }
  }
  if (!have_stats) {
    if ((rc = radix_pass(c, col, n, b.hist, b.offs, b.ka, b.ra)) != AH_OK) return rc;
    // how many rows of each category?  offs (inclusive scan, digit-major): the last tile's entry of digit d
    unsigned ends[3];
    for (int d = 0; d < 3; d++)
      AH_HIP(c, hipMemcpyAsync(&c->pinned[d], b.offs + ((int64_t)d + 1) * ntiles - 1, 4, hipMemcpyDeviceToHost, c->stream));
    AH_HIP(c, hipStreamSynchronize(c->stream));
    for (int d = 0; d < 3; d++) ends[d] = *(volatile unsigned*)&c->pinned[d];
    // the `rest` category is digit 0 (nulls at end) or digit 2 (nulls at start)
    rest_lo = nulls_at_start ? ends[1] : 0;
    rest_n = nulls_at_start ? (int64_t)ends[2] - ends[1] : ends[0];
  }
  unsigned long long *kcur = b.ka + rest_lo, *kalt = b.kb + rest_lo;
  unsigned *rcur = b.ra + rest_lo, *ralt = b.rb + rest_lo;
  if (rest_n > 1) {
    if (!have_stats) {
      // (2) which key bytes vary; smallest and largest key
      const unsigned agrid = std::min(ah_stream_grid(c, ah_ceil_div(rest_n, kBlock), 4), (unsigned)kAndOrGrid);
      and_or_kernel<<<agrid, kBlock, 0, c->stream>>>(kcur, rest_n, b.andor);
      AH_LAUNCH_CHECK(c);
      std::vector<unsigned long long> parts((size_t)agrid * 4);
      AH_HIP(c, hipMemcpyAsync(parts.data(), b.andor, parts.size() * 8, hipMemcpyDeviceToHost, c->stream));
      AH_HIP(c, hipStreamSynchronize(c->stream));
      for (unsigned g = 0; g < agrid; g++) {
        k_and &= parts[g * 4]; k_or |= parts[g * 4 + 1];
        kmin = parts[g * 4 + 2] < kmin ? parts[g * 4 + 2] : kmin;
        kmax = parts[g * 4 + 3] > kmax ? parts[g * 4 + 3] : kmax;
      }
    }
    const unsigned long long varying = k_and ^ k_or;
    int nvar = 0;
    for (int by = 0; by < (int)sizeof(T); by++) nvar += ((varying >> (8 * by)) & 0xFFull) != 0;
    // (3') large inputs with ≥ 4 varying bytes, in input order (the first key processed): two unstable MSD partition passes
    // + one wave per bucket comparing (key, row) — ah_sort_msd.hip.  Equal keys end up in row order = input order.
    bool done = false;
    if (rows_in == nullptr && nvar >= 4 && c->opt_sort_msd) {
      int used = -1;
      if ((rc = ah_sort_rest_msd(c, kcur, rcur, kalt, ralt, rest_n, varying, kmin, kmax, std::is_floating_point<T>::value ? (int)sizeof(T) : 0, descending, b.msd_tmp,
                                 (unsigned long long*)(rest_n == n ? b.final_out : nullptr), b.final_n, &used)) != AH_OK) return rc;
      if (used > 0) {
        done = true;   // sorted rows are in rcur (each bucket is rewritten in place) — or already widened in the output
        b.emitted = rest_n == n && b.final_out != nullptr;
      } else if (used == 0 && b.msd_tmp && ah_sort_msd_temp_bytes(rest_n) != 0) {
        // it ran and gave up (a bucket too large): the pairs are gone — pass (1) again, then the LSD passes
        if ((rc = radix_pass(c, col, n, b.hist, b.offs, b.ka, b.ra)) != AH_OK) return rc;
      }
    }
    // (3) one stable pass per varying byte, least significant first
    for (int by = 0; !done && by < (int)sizeof(T); by++) {
      if (((varying >> (8 * by)) & 0xFFull) == 0) continue;
      Pairs src{kcur, rcur, 8 * by};
      if ((rc = radix_pass(c, src, rest_n, b.hist, b.offs, kalt, ralt)) != AH_OK) return rc;
      unsigned long long* tk = kcur; kcur = kalt; kalt = tk;
      unsigned* tr = rcur; rcur = ralt; ralt = tr;
    }
    // the rest range must end up in ra, next to the NaN / null groups pass (1) left there
    if (!b.emitted && rcur != b.ra + rest_lo) AH_HIP(c, hipMemcpyAsync(b.ra + rest_lo, rcur, (size_t)rest_n * 4, hipMemcpyDeviceToDevice, c->stream));
  }
  return AH_OK;
}

int sort_dispatch(ah_ctx* c, SortBuffers& b, const SortCol& k, int64_t n, const unsigned* rows_in) {
  switch (k.type) {
#define AH_SORT(ID, T) case ID: return sort_by_column<T>(c, b, k.values, k.valid, k.off, n, k.descending, k.nulls_at_start, rows_in);
    AH_SORT(AH_UINT8, uint8_t) AH_SORT(AH_INT8, int8_t) AH_SORT(AH_UINT16, uint16_t) AH_SORT(AH_INT16, int16_t)
    AH_SORT(AH_UINT32, uint32_t) AH_SORT(AH_INT32, int32_t) AH_SORT(AH_UINT64, uint64_t) AH_SORT(AH_INT64, int64_t)
    AH_SORT(AH_FLOAT32, float) AH_SORT(AH_FLOAT64, double)
#undef AH_SORT
  }
  if (ah_sort_is_binary(k.type)) return ah_sort_by_binary(c, b, k, n, rows_in);
  return ah_fail(c, AH_ENOTIMPL, "sorting not supported for type %d", k.type);  // vector_sort.go:266-268
}

// rows0: the rows to order, n of them (NULL: rows 0 … n − 1).  Rows that tie on every key keep the order they have in rows0.
// head ≥ 0: only the first `head` (≤ n) entries of the order are written to `out`.
int sort_keys(ah_ctx* c, int nkeys, const SortCol* keys, int64_t n, uint64_t* out, const unsigned* rows0 = nullptr, int64_t head = -1) {
  SortBuffers b;
  const int64_t ntiles = ah_ceil_div(n, kTile);
  int rc;
  bool any_binary = false;
  for (int k = 0; k < nkeys; k++) any_binary |= ah_sort_is_binary(keys[k].type);
  const size_t hist_bytes = (size_t)kRadix * ntiles * 4;
  const size_t msd_bytes = c->opt_sort_msd ? ah_sort_msd_temp_bytes(n) : 0;   // sized for rest_n = n
  const size_t bin_bytes = any_binary ? kBinArrays * Carver::pad((size_t)n * 4) : 0;
  const size_t total = 2 * Carver::pad((size_t)n * 8) + (nkeys > 1 ? 3 : 2) * Carver::pad((size_t)n * 4) + 2 * Carver::pad(hist_bytes) + Carver::pad(4096 * 8 * 8) + Carver::pad(msd_bytes) + bin_bytes;
  void* arena;
  if ((rc = ah_temp_reserve(c, total, &arena)) != AH_OK) return rc;
  Carver tmp{(uint8_t*)arena};
  tmp.take((size_t)n * 8, &b.ka);
  tmp.take((size_t)n * 8, &b.kb);
  tmp.take((size_t)n * 4, &b.ra);
  tmp.take((size_t)n * 4, &b.rb);
  b.rc = nullptr;
  if (nkeys > 1) tmp.take((size_t)n * 4, &b.rc);
  tmp.take(hist_bytes, &b.hist);
  tmp.take(hist_bytes, &b.offs);
  tmp.take((size_t)kAndOrGrid * 8 * 8, &b.andor);   // ≤ kAndOrGrid workgroups × {AND, OR, min, max, NaNs} (8 words reserved each)
  if (msd_bytes) { uint8_t* m; tmp.take(msd_bytes, &m); b.msd_tmp = m; }
  if (any_binary)
    for (int i = 0; i < kBinArrays; i++) tmp.take((size_t)n * 4, &b.bin[i]);
  // lexicographic order by keys 0..k−1 = stable sorts by key k−1, …, key 0 in turn (every pass is stable)
  const unsigned* rows_in = rows0;
  if (nkeys == 1) { b.final_out = out; b.final_n = head < 0 ? n : head; }
  for (int k = nkeys - 1; k >= 0; k--) {
    if ((rc = sort_dispatch(c, b, keys[k], n, rows_in)) != AH_OK) return rc;
    if (k > 0) {
      AH_HIP(c, hipMemcpyAsync(b.rc, b.ra, (size_t)n * 4, hipMemcpyDeviceToDevice, c->stream));
      rows_in = b.rc;
    }
  }
  if (!b.emitted) {
    const int64_t written = head < 0 ? n : head;
    emit_kernel<<<ah_stream_grid(c, ah_ceil_div(written, kBlock), 8), kBlock, 0, c->stream>>>(b.ra, written, out);
    AH_LAUNCH_CHECK(c);
  }
  return AH_OK;
}

}  // namespace

int ah_partition_by_group(ah_ctx* c, const int32_t* ids, const unsigned long long* vals, const uint8_t* vvalid, int64_t voff, int64_t n, int shift,
                          int passes, unsigned* hist, unsigned* offs, unsigned long long* alt_vals, unsigned* alt_ids,
                          unsigned long long* out_vals, unsigned* out_ids) {
  IdVal src{ids, vals, vvalid, voff, shift};
  if (passes == 1) return radix_pass(c, src, n, hist, offs, out_vals, out_ids);
  int rc = radix_pass(c, src, n, hist, offs, alt_vals, alt_ids);
  if (rc != AH_OK) return rc;
  ValId src2{alt_vals, alt_ids, shift + 8};
  return radix_pass(c, src2, n, hist, offs, out_vals, out_ids);
}

int ah_sort_pairs_lsd(ah_ctx* c, unsigned long long* keys, unsigned* rows, unsigned long long* alt_keys, unsigned* alt_rows, int64_t n,
                      unsigned* hist, unsigned* offs, unsigned long long** sorted_keys) {
  for (int by = 0; by < 8; by++) {
    Pairs src{keys, rows, 8 * by};
    int rc = radix_pass(c, src, n, hist, offs, alt_keys, alt_rows);
    if (rc != AH_OK) return rc;
    unsigned long long* tk = keys; keys = alt_keys; alt_keys = tk;
    unsigned* tr = rows; rows = alt_rows; alt_rows = tr;
  }
  *sorted_keys = keys;
  return AH_OK;
}

static int check_column(ah_ctx* c, int type, const void* values) {
  const int w = ah_type_width(type);
  if (!w) return ah_fail(c, AH_ENOTIMPL, "sorting not supported for type %d", type);  // vector_sort.go:266-268
  if (!values) return ah_fail(c, AH_EINVALID, "sort_indices: null buffer");
  if ((uintptr_t)values & (uintptr_t)(w - 1)) return ah_fail(c, AH_EINVALID, "sort_indices: buffer not element-aligned");
  return AH_OK;
}

// a key of ah_sort_indices_keys → the driver's column; the buffers are checked as far as the host can
static int check_key(ah_ctx* c, const ah_sort_key& k, SortCol* col) {
  *col = SortCol{k.type, nullptr, nullptr, nullptr, 0, k.valid, k.off, k.descending, k.nulls_at_start};
  switch (k.type) {
    case AH_BINARY: case AH_LARGE_BINARY: {
      const int ow = k.type == AH_BINARY ? 4 : 8;
      if (!k.offsets) return ah_fail(c, AH_EINVALID, "sort_indices: null buffer");
      if ((uintptr_t)k.offsets & (uintptr_t)(ow - 1)) return ah_fail(c, AH_EINVALID, "sort_indices: buffer not element-aligned");
      col->offsets = k.offsets;
      col->data = (const uint8_t*)k.values;   // may be null when every value is empty: no byte is then read
      return AH_OK;
    }
    case AH_FIXED_SIZE_BINARY: case AH_DECIMAL128: case AH_DECIMAL256: {
      const int w = k.type == AH_DECIMAL128 ? 16 : k.type == AH_DECIMAL256 ? 32 : k.byte_width;
      if (k.byte_width != w || w < 1) return ah_fail(c, AH_EINVALID, "sort_indices: byte width %d does not fit type %d", k.byte_width, k.type);
      if (!k.values) return ah_fail(c, AH_EINVALID, "sort_indices: null buffer");
      col->data = (const uint8_t*)k.values;
      col->width = w;
      return AH_OK;
    }
  }
  const int rc = check_column(c, k.type, k.values);
  if (rc != AH_OK) return rc;
  col->values = (const uint8_t*)k.values + k.off * ah_type_width(k.type);
  return AH_OK;
}

int ah_sort_rows_keys(ah_ctx* c, int nkeys, const ah_sort_key* keys, const unsigned* rows, int64_t m, int64_t head, uint64_t* out_indices) {
  std::vector<SortCol> cols((size_t)nkeys);
  for (int k = 0; k < nkeys; k++) {
    const int rc = check_key(c, keys[k], &cols[k]);
    if (rc != AH_OK) return rc;
  }
  return m > 0 && head > 0 ? sort_keys(c, nkeys, cols.data(), m, out_indices, rows, head < m ? head : m) : AH_OK;
}

AH_EXPORT int ah_sort_indices(ah_ctx* c, int type, const void* values, const uint8_t* valid, int64_t off, int64_t n, int descending,
                              int nulls_at_start, uint64_t* out_indices) {
  return ah_sort_indices_multi(c, 1, &type, &values, &valid, &off, n, &descending, &nulls_at_start, out_indices);
}

AH_EXPORT int ah_sort_indices_multi(ah_ctx* c, int nkeys, const int* types, const void* const* values, const uint8_t* const* valids,
                                    const int64_t* offs, int64_t n, const int* descending, const int* nulls_at_start, uint64_t* out_indices) {
  AH_ENTER(c);
  if (nkeys < 1) return ah_fail(c, AH_EINVALID, "must provide at least one sort key");  // compute/vector_sort.go:119-121
  if (n < 0) return ah_fail(c, AH_EINVALID, "sort_indices: negative length");
  for (int k = 0; k < nkeys; k++)
    if (offs[k] < 0) return ah_fail(c, AH_EINVALID, "sort_indices: negative offset");
  if (n == 0) return AH_OK;
  if (!out_indices) return ah_fail(c, AH_EINVALID, "sort_indices: null buffer");
  if (n >= ((int64_t)1 << 32)) return ah_fail(c, AH_ENOTIMPL, "sort_indices: more than 2^32 - 1 rows in one batch");
  std::vector<SortCol> cols((size_t)nkeys);
  for (int k = 0; k < nkeys; k++) {
    int rc = check_column(c, types[k], values[k]);
    if (rc != AH_OK) return rc;
    cols[k] = SortCol{types[k], values[k], nullptr, nullptr, 0, valids[k], offs[k], descending[k], nulls_at_start[k]};
  }
  return sort_keys(c, nkeys, cols.data(), n, out_indices);
}

AH_EXPORT int ah_sort_indices_keys(ah_ctx* c, int nkeys, const ah_sort_key* keys, int64_t n, uint64_t* out_indices) {
  AH_ENTER(c);
  if (nkeys < 1) return ah_fail(c, AH_EINVALID, "must provide at least one sort key");  // compute/vector_sort.go:119-121
  if (!keys) return ah_fail(c, AH_EINVALID, "sort_indices: null buffer");
  if (n < 0) return ah_fail(c, AH_EINVALID, "sort_indices: negative length");
  for (int k = 0; k < nkeys; k++)
    if (keys[k].off < 0) return ah_fail(c, AH_EINVALID, "sort_indices: negative offset");
  if (n == 0) return AH_OK;
  if (!out_indices) return ah_fail(c, AH_EINVALID, "sort_indices: null buffer");
  if (n >= ((int64_t)1 << 32)) return ah_fail(c, AH_ENOTIMPL, "sort_indices: more than 2^32 - 1 rows in one batch");
  std::vector<SortCol> cols((size_t)nkeys);
  for (int k = 0; k < nkeys; k++) {
    const int rc = check_key(c, keys[k], &cols[k]);
    if (rc != AH_OK) return rc;
  }
  return sort_keys(c, nkeys, cols.data(), n, out_indices);
}
