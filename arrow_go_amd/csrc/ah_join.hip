// ah_join.hip — the kernels of hash_join over caller-supplied dense group ids: ah_join_build, ah_join_count, ah_join_expand,
// ah_join_match_bits.
//
// No reference analogue (arrow-go has no join); definitions in DESIGN.md §3.2a.  Both sides of a join carry the dense ids ONE
// ah_group_ids call gave their key tuples, so "equal keys" is "equal ids" and nothing here hashes or compares a key:
//   build   the build side's rows grouped by id — a CSR: starts[g] .. starts[g + 1] delimit, in `rows`, the valid rows of group g in
//           ascending row order.  Counts (ah_group_count) → exclusive scan (ah_cumulative_sum) → the existing STABLE sort on the ids;
//           a row under a cleared validity bit sorts with the key `ngroups`, behind every group.
//   count   m[i] = the length of probe row i's group (0 under a cleared validity bit; at least 1 for a left outer join), scanned into
//           offsets[0 .. n_probe]; the total goes home to the host, which sizes the result with it.
//   expand  the hot path: output slot j belongs to the probe row i with offsets[i] <= j < offsets[i + 1].  Parallel over OUTPUT SLOTS:
//           a workgroup owns kExpandTile consecutive slots whatever the run lengths are, so one probe row with a million matches and
//           a million probe rows with one match each are the same work per output row.
//   match   bit i = probe row i is valid and its group is not empty: the mask of a semi join, inverted that of an anti join.
//
// join_expand_kernel, per workgroup:
//   1. two waves find, each with a 64-ary search in `offsets` (one load per lane and step, 4 steps for 2^24 rows), the probe rows
//      i_lo and i_hi that own the tile's first and last slot;
//   2. the slice offsets[i_lo .. i_hi + 1] is read once, coalesced, and every NON-EMPTY row leaves in LDS, at the tile position where
//      its run starts (clamped to 0 for a run that began in an earlier tile), a marker: its row number and `starts[id] − offsets[i]`,
//      the constant that turns a slot number into a position in `rows`.  Empty rows leave nothing: they are skipped for good;
//   3. a max-scan over the marker positions (8 slots per lane, shuffles across the wave, 4 words across the waves) tells every slot
//      which marker it belongs to — a run that spans the whole tile is one marker at position 0;
//   4. every lane writes 2 consecutive slots = 16 bytes of each index vector per store, 4 stores per vector, the 8 gathers from
//      `rows` (the only irregular access; consecutive inside a run) issued before the first store.
//   The validity bits of a left outer join are written in step 3, where a lane owns exactly one byte; a tile is a multiple of 64
//   slots, so no two workgroups share a byte.  No atomics, no look-back, no spinning: a tile depends on the inputs alone.
//   LDS: 32 KiB per workgroup (2 × 4 B + 8 B per slot) — 5 workgroups = 20 waves per CU.
// HBM per call: 8 B per probe row of offsets + 4 B of ids (+ 8 – 16 B of `starts` per non-empty row), 8 B per slot from `rows`, 16 B
// per slot written.
#include "ah_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kExpandTile = 2048;          // output slots per workgroup of join_expand_kernel
constexpr int kSlotsPerLane = kExpandTile / kBlock;
static_assert(kSlotsPerLane == 8, "a lane owns one byte of the validity bitmap and 4 x 2 slots of the stores");
constexpr long long kUnmatched = (long long)0x8000000000000000ull;   // a marker's base: the run is one slot without a build row

// keys[i] = ids[i], or `ngroups` under a cleared validity bit: the sort then needs no null handling and puts those rows last
__global__ __launch_bounds__(kBlock) void join_mask_ids_kernel(const int32_t* __restrict__ ids, const uint8_t* __restrict__ valid, int64_t voff, int64_t n,
                                                                int32_t ngroups, int32_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = ah_bit(valid, voff + i) ? ids[i] : ngroups;
}

__global__ __launch_bounds__(kBlock) void join_count_kernel(const int32_t* __restrict__ ids, const uint8_t* __restrict__ valid, int64_t poff, int64_t n,
                                                             const int64_t* __restrict__ starts, int emit_unmatched, int64_t* __restrict__ m) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    int64_t c = 0;
    if (ah_bit(valid, poff + i)) {
      const int32_t g = ids[i];
      c = starts[g + 1] - starts[g];
    }
    m[i] = c == 0 && emit_unmatched ? 1 : c;
  }
}

// one wave per 64 probe rows: the ballot is the chunk's eight bytes
__global__ __launch_bounds__(kBlock) void join_match_bits_kernel(const int32_t* __restrict__ ids, const uint8_t* __restrict__ valid, int64_t poff, int64_t n,
                                                                  const int64_t* __restrict__ starts, uint8_t* __restrict__ out) {
  const int64_t nchunks = (n + 63) >> 6, stride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t chunk = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); chunk < nchunks; chunk += stride) {
    const int64_t i = chunk * 64 + ah_lane();
    bool hit = false;
    if (i < n && ah_bit(valid, poff + i)) {
      const int32_t g = ids[i];
      hit = starts[g + 1] > starts[g];
    }
    const unsigned long long word = __ballot(hit);
    if (ah_lane() == 0) put_chunk_bytes(out, chunk, n, word);
  }
}

// The first index in [0, n) with a[index] > key, n if there is none; `a` does not descend.  Called by a whole wave with the same
// arguments: every step probes 64 evenly spaced entries at once and keeps the one gap the answer lies in.
__device__ __forceinline__ int64_t wave_upper_bound(const int64_t* __restrict__ a, int64_t n, int64_t key) {
  int64_t lo = 0, hi = n;   // the answer is in [lo, hi]; hi == n or a[hi] > key
  const int lane = ah_lane();
  while (lo < hi) {
    const int64_t step = (hi - lo + 63) >> 6;
    const int64_t at = lo + (int64_t)(lane + 1) * step - 1;   // lane 63 reaches hi − 1 or beyond
    const bool greater = at >= hi || a[at] > key;
    const unsigned long long b = __ballot(greater);
    if (b == 0) return hi;                                    // every entry of [lo, hi) is <= key
    const int f = __ffsll(b) - 1;                             // the lanes below f saw entries <= key
    const int64_t first = lo + (int64_t)(f + 1) * step - 1;
    lo += (int64_t)f * step;
    hi = first < hi ? first : hi;
  }
  return lo;
}

__global__ __launch_bounds__(kBlock) void join_expand_kernel(const int32_t* __restrict__ ids, const uint8_t* __restrict__ pvalid, int64_t poff, int64_t n_probe,
                                                              const int64_t* __restrict__ starts, const int64_t* __restrict__ rows,
                                                              const int64_t* __restrict__ offsets, int64_t total, int64_t* __restrict__ out_probe,
                                                              int64_t* __restrict__ out_build, uint8_t* __restrict__ out_valid, int aligned) {
  __shared__ int s_mark[kExpandTile];         // step 2: the slot's own position where a run starts, −1 elsewhere; step 3: the slot's marker
  __shared__ int s_rel[kExpandTile];          // at a marker: the probe row, relative to i_lo
  __shared__ long long s_base[kExpandTile];   // at a marker: starts[id] − offsets[row], or kUnmatched
  __shared__ long long s_bounds[2];
  __shared__ int s_wave[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t j0 = (int64_t)blockIdx.x * kExpandTile;
  const int cnt = total - j0 < kExpandTile ? (int)(total - j0) : kExpandTile;   // >= 1: the grid covers `total` slots
  // 1. the probe rows of the first and of the last slot: the last i with offsets[i] <= j, which is not empty
  if (wave < 2) {
    const int64_t i = wave_upper_bound(offsets, n_probe + 1, wave == 0 ? j0 : j0 + cnt - 1) - 1;
    if (lane == 0) s_bounds[wave] = i;
  }
#pragma unroll
  for (int k = 0; k < kSlotsPerLane; k++) s_mark[tid + k * kBlock] = -1;
  __syncthreads();
  const int64_t i_lo = s_bounds[0], i_hi = s_bounds[1];
  // 2. the markers.  Row i_lo holds slot j0, so position 0 always gets one; every later run starts inside the tile at a place of its own
  for (int64_t i = i_lo + tid; i <= i_hi; i += kBlock) {
    const int64_t o0 = offsets[i], o1 = offsets[i + 1];
    if (o1 <= o0) continue;
    long long base = kUnmatched;
    if (ah_bit(pvalid, poff + i)) {
      const int32_t g = ids[i];
      const int64_t s0 = starts[g];
      if (starts[g + 1] > s0) base = s0 - o0;
    }
    const int pos = o0 > j0 ? (int)(o0 - j0) : 0;
    s_mark[pos] = pos;
    s_rel[pos] = (int)(i - i_lo);
    s_base[pos] = base;
  }
  __syncthreads();
  // 3. every slot's marker = the largest marker position at or before it; a lane owns slots [8 tid, 8 tid + 8) = one validity byte
  int m[kSlotsPerLane];
  int run = -1;
#pragma unroll
  for (int k = 0; k < kSlotsPerLane; k++) {
    const int v = s_mark[tid * kSlotsPerLane + k];
    run = v > run ? v : run;
    m[k] = run;
  }
  int inc = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc = t > inc ? t : inc;
  }
  if (lane == 63) s_wave[wave] = inc;
  int before = __shfl_up(inc, 1, 64);
  if (lane == 0) before = -1;
  __syncthreads();
  for (int w = 0; w < wave; w++) before = s_wave[w] > before ? s_wave[w] : before;
  unsigned vbyte = 0;
#pragma unroll
  for (int k = 0; k < kSlotsPerLane; k++) {
    const int p = m[k] > before ? m[k] : before;   // >= 0: position 0 holds a marker
    s_mark[tid * kSlotsPerLane + k] = p;
    if (tid * kSlotsPerLane + k < cnt && s_base[p] != kUnmatched) vbyte |= 1u << k;
  }
  if (out_valid && tid * kSlotsPerLane < cnt) out_valid[(j0 >> 3) + tid] = (uint8_t)vbyte;   // bits at and above `total`: 0
  __syncthreads();
  // 4. the two index vectors: 2 slots per lane and store, the gathers first
  int64_t prow[kSlotsPerLane], brow[kSlotsPerLane];
#pragma unroll
  for (int u = 0; u < kSlotsPerLane / 2; u++) {
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const int q = u * 2 * kBlock + 2 * tid + e;
      const int p = s_mark[q];
      const long long base = s_base[p];
      prow[2 * u + e] = i_lo + s_rel[p];
      brow[2 * u + e] = q < cnt && base != kUnmatched ? rows[base + (j0 + q)] : 0;
    }
  }
#pragma unroll
  for (int u = 0; u < kSlotsPerLane / 2; u++) {
    const int q = u * 2 * kBlock + 2 * tid;
    if (q + 1 < cnt) {
      ah_vec16<int64_t> a, b;
      a.v[0] = prow[2 * u]; a.v[1] = prow[2 * u + 1];
      b.v[0] = brow[2 * u]; b.v[1] = brow[2 * u + 1];
      ah_store16<int64_t>(out_probe, (j0 + q) >> 1, a, aligned);
      ah_store16<int64_t>(out_build, (j0 + q) >> 1, b, aligned);
    } else if (q < cnt) {   // the last slot of an odd total
      out_probe[j0 + q] = prow[2 * u];
      out_build[j0 + q] = brow[2 * u];
    }
  }
}

// what the four entry points check alike: lengths and offsets, the row limit of the id-based aggregates
int join_check(ah_ctx* c, const char* who, int64_t n, int64_t off) {
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "%s: negative length/offset", who);
  if (n > ((int64_t)1 << 30)) return ah_fail(c, AH_ENOTIMPL, "%s: more than 2^30 rows per call", who);
  return AH_OK;
}

}  // namespace

AH_EXPORT int ah_join_build(ah_ctx* c, const int32_t* build_ids, const uint8_t* build_valid, int64_t voff, int64_t n_build, int64_t ngroups,
                            int64_t* out_starts, int64_t* out_rows) {
  AH_ENTER(c);
  int rc = join_check(c, "join_build", n_build, voff);
  if (rc != AH_OK) return rc;
  if (ngroups < 0) return ah_fail(c, AH_EINVALID, "join_build: negative length/offset");
  if (ngroups >= 0x7fffffffll) return ah_fail(c, AH_EINVALID, "join_build: more than 2^31 - 2 groups");
  if (!out_starts) return ah_fail(c, AH_EINVALID, "join_build: null buffer");
  if (n_build > 0 && ngroups == 0) return ah_fail(c, AH_EINVALID, "join_build: rows but no groups");
  if (n_build == 0) {   // every group is empty
    AH_HIP(c, hipMemsetAsync(out_starts, 0, (size_t)(ngroups + 1) * sizeof(int64_t), c->stream));
    return AH_OK;
  }
  if (!build_ids || !out_rows) return ah_fail(c, AH_EINVALID, "join_build: null buffer");
  // the groups' sizes, counted over the valid rows, and their exclusive scan: starts[0] = 0, starts[g + 1] = the inclusive sum
  void* counts = nullptr;
  if ((rc = ah_temp_reserve(c, ah_pad((size_t)ngroups * sizeof(int64_t)), &counts)) != AH_OK) return rc;
  if ((rc = ah_group_count(c, build_ids, ngroups, build_valid, voff, n_build, (int64_t*)counts)) != AH_OK) return rc;
  AH_HIP(c, hipMemsetAsync(out_starts, 0, sizeof(int64_t), c->stream));
  if ((rc = ah_cumulative_sum(c, AH_INT64, counts, nullptr, 0, ngroups, nullptr, 0, 0, out_starts + 1, nullptr, nullptr)) != AH_OK) return rc;
  // the rows by group, ties in row order: the stable sort on the ids.  The sort takes the temp arena (the counts are through with it:
  // the scan is ahead of it on the stream), so the masked copy of the ids lives in the packed-key block, which the sort leaves alone.
  const int32_t* keys = build_ids;
  if (build_valid) {
    void* masked = nullptr;
    if ((rc = ah_pack_reserve(c, (size_t)n_build * sizeof(int32_t), &masked)) != AH_OK) return rc;
    join_mask_ids_kernel<<<ah_stream_grid(c, ah_ceil_div(n_build, kBlock)), kBlock, 0, c->stream>>>(build_ids, build_valid, voff, n_build, (int32_t)ngroups,
                                                                                                     (int32_t*)masked);
    AH_LAUNCH_CHECK(c);
    keys = (const int32_t*)masked;
  }
  return ah_sort_indices(c, AH_INT32, keys, nullptr, 0, n_build, 0, 0, (uint64_t*)out_rows);
}

AH_EXPORT int ah_join_count(ah_ctx* c, const int32_t* probe_ids, const uint8_t* probe_valid, int64_t poff, int64_t n_probe, const int64_t* starts,
                            int emit_unmatched, int64_t* out_offsets, int64_t* out_total_host) {
  AH_ENTER(c);
  if (out_total_host) *out_total_host = 0;
  int rc = join_check(c, "join_count", n_probe, poff);
  if (rc != AH_OK) return rc;
  if (!out_offsets || !out_total_host) return ah_fail(c, AH_EINVALID, "join_count: null buffer");
  AH_HIP(c, hipMemsetAsync(out_offsets, 0, sizeof(int64_t), c->stream));
  if (n_probe == 0) return AH_OK;
  if (!probe_ids || !starts) return ah_fail(c, AH_EINVALID, "join_count: null buffer");
  void* m = nullptr;
  if ((rc = ah_temp_reserve(c, ah_pad((size_t)n_probe * sizeof(int64_t)), &m)) != AH_OK) return rc;
  join_count_kernel<<<ah_stream_grid(c, ah_ceil_div(n_probe, kBlock)), kBlock, 0, c->stream>>>(probe_ids, probe_valid, poff, n_probe, starts,
                                                                                               emit_unmatched ? 1 : 0, (int64_t*)m);
  AH_LAUNCH_CHECK(c);
  if ((rc = ah_cumulative_sum(c, AH_INT64, m, nullptr, 0, n_probe, nullptr, 0, 0, out_offsets + 1, nullptr, nullptr)) != AH_OK) return rc;
  AH_HIP(c, hipMemcpyAsync(c->pinned, out_offsets + n_probe, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipStreamSynchronize(c->stream));
  *out_total_host = *(volatile int64_t*)c->pinned;
  return AH_OK;
}

AH_EXPORT int ah_join_expand(ah_ctx* c, const int32_t* probe_ids, const uint8_t* probe_valid, int64_t poff, int64_t n_probe, const int64_t* starts,
                             const int64_t* rows, const int64_t* offsets, int64_t total, int emit_unmatched, int64_t* out_probe_rows,
                             int64_t* out_build_rows, uint8_t* out_build_valid, int64_t* out_null_count_host) {
  AH_ENTER(c);
  if (out_null_count_host) *out_null_count_host = 0;
  int rc = join_check(c, "join_expand", n_probe, poff);
  if (rc != AH_OK) return rc;
  if (total < 0) return ah_fail(c, AH_EINVALID, "join_expand: negative length/offset");
  if (total > ((int64_t)1 << 40)) return ah_fail(c, AH_ENOTIMPL, "join_expand: more than 2^40 output rows per call");
  if (total == 0) return AH_OK;
  if (n_probe == 0) return ah_fail(c, AH_EINVALID, "join_expand: output rows but no probe rows");
  if (!probe_ids || !starts || !offsets || !out_probe_rows || !out_build_rows || (emit_unmatched && !out_build_valid))
    return ah_fail(c, AH_EINVALID, "join_expand: null buffer");
  const int aligned = (((uintptr_t)out_probe_rows | (uintptr_t)out_build_rows) & 15) == 0;
  join_expand_kernel<<<(unsigned)ah_ceil_div(total, kExpandTile), kBlock, 0, c->stream>>>(probe_ids, probe_valid, poff, n_probe, starts, rows, offsets, total,
                                                                                          out_probe_rows, out_build_rows,
                                                                                          emit_unmatched ? out_build_valid : nullptr, aligned);
  AH_LAUNCH_CHECK(c);
  if (emit_unmatched && out_null_count_host) {   // the bitmap was just written: its popcount reads 1/192 of what the kernel moved
    int64_t set = 0;
    if ((rc = ah_count_set_bits(c, out_build_valid, 0, total, &set)) != AH_OK) return rc;
    *out_null_count_host = total - set;
  }
  return AH_OK;
}

AH_EXPORT int ah_join_match_bits(ah_ctx* c, const int32_t* probe_ids, const uint8_t* probe_valid, int64_t poff, int64_t n_probe, const int64_t* starts,
                                 uint8_t* out_bits) {
  AH_ENTER(c);
  int rc = join_check(c, "join_match_bits", n_probe, poff);
  if (rc != AH_OK) return rc;
  if (n_probe == 0) return AH_OK;
  if (!probe_ids || !starts || !out_bits) return ah_fail(c, AH_EINVALID, "join_match_bits: null buffer");
  join_match_bits_kernel<<<ah_stream_grid(c, ah_ceil_div(n_probe, kBlock)), kBlock, 0, c->stream>>>(probe_ids, probe_valid, poff, n_probe, starts, out_bits);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}
