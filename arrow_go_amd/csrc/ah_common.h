// ah_common.h — shared host/device helpers for libarrowhip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <initializer_list>
#include <type_traits>
#include <stdarg.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/arrowhip.h"

#define AH_EXPORT extern "C" __attribute__((visibility("default")))

// What ah_filter_count leaves for the ah_filter_primitive that follows it (the two-phase protocol of
// vector_selection.go:459/475: count, allocate, fill): the per-tile survivor prefixes of THAT mask, so the fill does not
// count the selection vector a second time.  Dropped by every entry point that may change device memory (AH_ENTER);
// allocation, synchronisation, timers and a memset / upload / copy that stays clear of the mask's bytes keep it (AH_ENTER_KEEP).
struct ah_filter_cache {
  bool valid;
  const uint8_t *fdata, *fvalid;
  int64_t foff, n, ntiles;
  int null_sel, tile_rows;
  void* buf;          // device: super_off[nsuper] (int64) | tile_local[ntiles] (int) | super_total[nsuper] (int) | total (int64)
  size_t bytes;
  int64_t* super_off;
  int* tile_local;
  int64_t* total;
};

struct ah_ctx {
  int device;
  hipStream_t stream;       // compute stream
  hipStream_t copy_stream;  // uploads / downloads
  bool owns_stream;
  hipEvent_t ev_copy;       // orders copy stream <-> compute stream
  hipEvent_t ev_compute;
  hipEvent_t t0, t1;        // ah_timer_*
  hipEvent_t* marks;        // ah_event_record ring (lazily created)
  int n_marks;
  // scratch arena (device): partial sums, tile counts, hash tables ...
  void* scratch;
  size_t scratch_bytes;
  void* temp;              // second grow-only arena: the temporaries of sort / group-by / var-length take (see ah_temp_reserve)
  size_t temp_bytes;
  void* pack;              // third grow-only block: the packed key column of ah_group_ids (see ah_pack_reserve)
  size_t pack_bytes;
  // small pinned staging block for *_host results (64 x 8 bytes)
  uint64_t* pinned;
  // small device block for scalar results / flags (64 x 8 bytes) followed by a
  // 4096-entry partials area (popcount)
  uint64_t* dscalars;
  int num_cu;
  // tunables (env ARROWHIP_NT / ARROWHIP_BLOCKS_PER_CU, read at ctx creation)
  int tune_nt;             // 1: nontemporal loads/stores on streaming kernels
  int tune_blocks_per_cu;  // grid cap for grid-stride streaming kernels
  // take (ah_take_binned.hip): ARROWHIP_TAKE_BINNED 0 never / 1 auto / 2 whenever legal; _WINDOW_LOG2 bytes of `values` per
  // bin; _GATHER_WG_PER_CU occupancy cap of the gather pass.  Also settable per context: ah_ctx_set_option.
  int opt_take_binned, opt_take_window_log2, opt_take_gather_wg, opt_take_gather_load, opt_take_gather_lds;
  int opt_groupby_keys;        // hash + sum: expected keys per partition the cut aims at (ARROWHIP_GROUPBY_KEYS; the LDS table admits 3584)
  int opt_groupby_partition;   // hash + sum (ah_groupby.hip): 0 never, 1 auto, k ≥ 2 always with 2^(k−2) partitions (ARROWHIP_GROUPBY_PARTITION)
  int opt_encode_partition;    // unique / dictionary_encode (ah_hash_part.hip): 0 never, 1 auto (by the prefix's distinct count), k ≥ 3: always, 2^k partitions (ARROWHIP_ENCODE_PARTITION)
  int opt_encode_part_slots;   // measurement: LDS table size of the one-cut path (8192 default, 4096)
  int opt_encode_byte_map;     // partition-first encode: first occurrences marked by plain byte stores into a byte map that one pass packs into the bitmap (1) or by device-scope atomicOr on the bitmap's words (0)
  int opt_encode_early_look;   // 1 (default): calls of ≥ 2^24 rows count the first 2^16 rows' distinct keys BEFORE the global table is set up (ah_encode_first_look); 0: the look that falls out of the staged inserts
  int opt_encode_part_min;     // auto: smallest expected distinct count that takes the partition-first path (ARROWHIP_ENCODE_PART_MIN)
  int opt_hash_direct;         // unique / dictionary_encode (ah_hash.hip): 0 ids in a separate pass, 1 direct ids, 2 + LDS / re-packed table (default), 3 no re-packed table (ARROWHIP_HASH_DIRECT)
  int opt_hash_sum_partition;  // id-based group-by sum above 4096 groups (ah_hash_agg.hip): 1 (default) partition the (value, id) pairs by id and aggregate run by run in LDS, 0 plain device atomics (ARROWHIP_HASH_PARTITION)
  int opt_sort_msd;            // sort_indices: 0 LSD passes only, 1 auto (ARROWHIP_SORT_MSD)
  int opt_scan_segment_log2;   // cumulative_sum: bytes of input per segment (ARROWHIP_SCAN_SEGMENT_LOG2; 0 = one segment)
  void* expr_cache;        // compiled expression programs (ah_expr.hip)
  int capturing;           // between ah_graph_begin and ah_graph_end: the compute stream records instead of running
  ah_filter_cache fcache;  // ah_filter.hip
  int opt_scan_onepass;    // cumulative_sum of 4- and 8-byte integers (checked or not, nulls or not): 1 (default) one pass with decoupled look-back over 128 KiB tiles, 0 reduce-then-scan, 2 one pass + separate validity copy / popcount, 3 one pass for unchecked columns without nulls only
  void* scan_recs;         // … its tile records (only that kernel writes them: stale words carry older epochs) and, in the last 64 bytes, its ticket word
  size_t scan_recs_bytes;
  unsigned scan_epoch;
  int opt_groupby_seed;    // direct group-by: 1 (default) the workgroups' LDS tables start from the quick look's keys and are added up slot by slot, 0 empty tables merged with atomics
  int opt_groupby_reserve; // partitioned group-by: 1 (default) the scatter reserves its runs in per-(partition, XCD) regions sized from the sample — no histogram pass —, 0 histogram → offsets → scatter
  int opt_groupby_lean;    // direct group-by: 0 always keep a pending group per lane, 1 (default) leave it out when the quick look says neighbouring rows rarely share a key, 2 always leave it out, 3 also in the partitioned path's aggregate pass (an experiment switch: −3 % on evenly spread keys, profiles/r06_gb_lean.json; a hot key would serialise its partition's LDS atomics)
  int opt_filter_cache;    // 1: ah_filter_count leaves its tile prefixes for the fill (default on a stream of the context's own), 0: the fill recounts (default on a shared stream)
  int take_clustered_hint; // ah_take_binned_try → ah_take.hip: this call's indices looked clustered (1), not (0); option take_vec: 0 never, 1 by the sample, 2 always
  int opt_take_vec;
  // The neighbour sample of the last Take (ah_take_binned_try), kept for the next call with the SAME index vector — a record batch's
  // columns are gathered one after the other with one index vector (compute/selection.go:601-677), and the sample + its wait were
  // ≈ 20 µs of every one of those calls.  Kept like the filter cache: valid only for the Take that directly follows (every other
  // compute entry point of this context drops it, an upload / copy / memset into the vector's bytes drops it, a Take whose outputs
  // overlap the vector does not leave one), off by default on a shared stream, sampled again on every 32nd use.  Every Take path
  // returns the same bytes (tests force each of them): an entry gone stale behind the library's back costs speed, never results.
  // Option take_hint_cache.
  bool take_hint_valid, take_hint_live;   // left by the last call / readable by this one (read before AH_ENTER drops it)
  const void* take_hint_idx; int64_t take_hint_nidx; int take_hint_kind, take_hint_near, take_hint_uses, opt_take_hint_cache;
  unsigned long long take_hint_word;
  int opt_arith_xcd_map;        // element-wise binary kernels: every XCD streams one contiguous eighth of the columns (1) or the blocks' natural interleave (0)
  int opt_groupby_scale_guess;  // no-cut Float64 group-by: fixed-point scale from a sample, verified by the aggregate pass (1) or from a pass over all values (0)
  int opt_encode_unperm2_group; // two-cut encode: the level-2 un-permute over 4 consecutive virtual tiles per workgroup (4, the default) or one per workgroup (0)
  int opt_encode_resolve_wgs;   // partition-first encode: workgroups of the resolve pass (partitions are split to reach it)
  int opt_encode_dict_compact;  // partition-first encode: the dictionary = the key column compacted by the first-occurrence bitmap (0 never, 1 from 1024 partitions on, 2 always)
  int opt_encode_table_batch;   // partition-first encode: the table pass probes its four records' first groups together (1) or one by one (0)
  int opt_encode_unperm_group;  // partition-first encode: tiles per workgroup in the final un-permute (1 or 4)
  int opt_take_vec_nt;     // nontemporal hints of the clustered take (7 all, 5 index + output, 4 output, 0 none)
  int opt_string_tile_bytes;  // string searches (ah_string_match.hip): bytes of the data buffer per LDS tile, 0 = the default (16384); 64 … 32768
  // 2 × 8 words of coherent (fine-grained) pinned host memory kernels can store to: {value, sequence number} for ah_filter_count, {≤ 7 words, sequence number} for ah_mailbox_read.  A count the host
  // must see before it can go on (ah_filter_count) is polled here instead of paying a stream synchronisation's wake-up.
  unsigned long long* mailbox;
  unsigned long long mailbox_seq;
  char err[512];
};

// grid size for a grid-stride streaming kernel over `work_items` block-iterations.
// default_bpc: the kernel's own default cap in workgroups per CU (0 = no cap: one
// iteration per workgroup, measured fastest for pure element-wise streams — 6.4-6.5 TB/s
// vs 6.0 with 8/CU, scripts/micro/add_variants.hip); ARROWHIP_BLOCKS_PER_CU overrides.
static inline unsigned ah_stream_grid(const ah_ctx* c, int64_t work_items, int default_bpc = 8) {
  int bpc = c->tune_blocks_per_cu > 0 ? c->tune_blocks_per_cu : default_bpc;
  int64_t cap = bpc > 0 ? (int64_t)c->num_cu * bpc : ((int64_t)1 << 30);
  int64_t g = work_items < cap ? work_items : cap;
  return (unsigned)(g < 1 ? 1 : g);
}

// ---- host-side error plumbing ------------------------------------------------
static inline int ah_fail(ah_ctx* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
static inline int ah_fail(ah_ctx* ctx, int code, const char* fmt, ...) {
  if (ctx) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

#define AH_HIP(ctx, call)                                                              \
  do {                                                                                 \
    hipError_t e__ = (call);                                                           \
    if (e__ != hipSuccess)                                                             \
      return ah_fail((ctx), AH_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                     __FILE__, __LINE__);                                              \
  } while (0)

#define AH_ENTER_KEEP(ctx)                                             \
  do {                                                                 \
    if (!(ctx)) return AH_EINVALID;                                    \
    (ctx)->err[0] = 0;                                                 \
    AH_HIP((ctx), hipSetDevice((ctx)->device));                        \
  } while (0)

#define AH_ENTER(ctx)                                                  \
  do {                                                                 \
    AH_ENTER_KEEP(ctx);                                                \
    (ctx)->fcache.valid = false;                                       \
    (ctx)->take_hint_valid = false;                                    \
  } while (0)

// does a write to [p, p + nbytes) touch the index vector the Take's path sample was taken from?
static inline bool ah_take_hint_overlaps(const ah_ctx* c, const void* p, size_t nbytes) {
  if (!c->take_hint_valid || !c->take_hint_idx) return false;
  const uintptr_t a = (uintptr_t)p, b = a + nbytes, lo = (uintptr_t)c->take_hint_idx, hi = lo + (size_t)c->take_hint_nidx * (size_t)(c->take_hint_kind / 2);
  return a < hi && lo < b;
}
// does a write to [p, p + nbytes) touch the mask the filter cache was computed from?
static inline bool ah_fcache_overlaps(const ah_ctx* c, const void* p, size_t nbytes) {
  if (!c->fcache.valid) return false;
  const uintptr_t a = (uintptr_t)p, b = a + nbytes;
  const uintptr_t lo = (uintptr_t)(c->fcache.foff >> 3), hi = (uintptr_t)((c->fcache.foff + c->fcache.n + 7) >> 3);
  for (const uint8_t* bm : {c->fcache.fdata, c->fcache.fvalid})
    if (bm && a < (uintptr_t)bm + hi && (uintptr_t)bm + lo < b) return true;
  return false;
}

#define AH_LAUNCH_CHECK(ctx) AH_HIP((ctx), hipGetLastError())

void ah_expr_cache_free(ah_ctx* ctx);  // ah_expr.hip
// internal (ah_arith.hip): the unchecked add / subtract / multiply of any shape — what the checked names are for floats
int ah_arith_binary(ah_ctx* ctx, int type, int op, int shape, const void* l, const void* r, void* out, int64_t len);
// internal (ah_sort.hip): stable radix partition of (value bits, group id) pairs for the group-by of
// ah_hash_agg.hip — by (id >> shift) & 255 (passes = 1) or by (id >> shift) & 65535 (passes = 2, LSD; alt_*
// is the intermediate buffer).  A row whose value is null (vvalid bit clear) travels with bit 31 of
// its id set.  hist / offs: 256 · ceil(n / 2048) unsigned each.
int ah_partition_by_group(ah_ctx* ctx, const int32_t* ids, const unsigned long long* vals, const uint8_t* vvalid, int64_t voff, int64_t n,
                          int shift, int passes, unsigned* hist, unsigned* offs, unsigned long long* alt_vals, unsigned* alt_ids,
                          unsigned long long* out_vals, unsigned* out_ids);
// internal (ah_sort_msd.hip): the `rest` range of sort_indices by two MSD partition passes + one wave per bucket; *used = 0: not
// applicable or a bucket came out too large — the pairs are clobbered and the caller regenerates them for the LSD passes
int ah_sort_rest_msd(ah_ctx* ctx, unsigned long long* keys, unsigned* rows, unsigned long long* alt_keys, unsigned* alt_rows, int64_t n,
                     unsigned long long varying, unsigned long long kmin, unsigned long long kmax, int float_bytes, int descending, void* tmp,
                     unsigned long long* out64, int64_t out64_n, int* used);
size_t ah_sort_msd_temp_bytes(int64_t n);   // size of `tmp`; 0: the path does not apply to n pairs
// internal (ah_sort.hip): (key, row) pairs sorted by the full 64-bit key with the stable LSD passes; *sorted_keys = where the keys ended up
int ah_sort_pairs_lsd(ah_ctx* ctx, unsigned long long* keys, unsigned* rows, unsigned long long* alt_keys, unsigned* alt_rows, int64_t n,
                      unsigned* hist, unsigned* offs, unsigned long long** sorted_keys);
// internal (ah_sort.hip): the m rows `rows` (row numbers of the keys' columns, not in the temp arena; NULL: rows 0 … m − 1)
// ordered by the keys as ah_sort_indices_keys orders all rows, the first min(head, m) entries of the order written; rows that
// tie on every key keep their order in `rows`.  Takes the temp arena.  The keys are checked as ah_sort_indices_keys checks them.
int ah_sort_rows_keys(ah_ctx* ctx, int nkeys, const ah_sort_key* keys, const unsigned* rows, int64_t m, int64_t head, uint64_t* out_indices);
// internal (ah_take_binned.hip): Take for random indices into a column the caches cannot hold; *used says whether it ran
int ah_take_binned_try(ah_ctx* ctx, int byte_width, const void* values, const uint8_t* vvalid, int64_t voff, int64_t nvalues, int iw,
                       int is_signed, const void* idx, const uint8_t* ivalid, int64_t ioff, int64_t nidx, void* out_values,
                       uint8_t* out_valid, unsigned long long* first_bad, int* used);
// internal (ah_groupby.hip): partition-first group-by; *used says whether it produced the result (else: the id-based path)
int ah_groupby_partitioned_try(ah_ctx* ctx, int is_f64, const uint64_t* keys, const uint8_t* kvalid, int64_t koff, const void* vals,
                               const uint8_t* vvalid, int64_t voff, int64_t n, uint64_t* out_keys, void* out_sums, int64_t* out_counts,
                               int64_t* out_first_rows, int64_t* out_ngroups, int32_t* out_null_group, int* used);
// internal (ah_sum.hip): the workgroup partials of one chunk written to a caller-owned array (16 bytes reserved per partial; *n_written
// counts 8-byte partials for the integer sums, 16-byte ones for Float64), and the one final reduction over all of them
int ah_fused_f64_parts_dev(ah_ctx* ctx, int cmpop, const double* x, const uint8_t* valid, int64_t off, int64_t n, double threshold,
                           double* out_sum_dev, int64_t* out_count_dev, double* out_parts_dev);
size_t ah_sum_partial_bytes(int is_f64);
int ah_sum_chunk_partials(ah_ctx* ctx, int is_f64, const void* buf, size_t len, void* partials, int max_partials, int* n_written);
int ah_sum_finish_partials(ah_ctx* ctx, int is_f64, const void* partials, int n, void* res_dev);
int ah_sum_short_f64(ah_ctx* ctx, const void* buf, size_t len, void* res_dev);   // ≤ 31 rows: the reference's sequential order
// internal (ah_hash_part.hip): unique / dictionary_encode of 8-byte keys by partitions of the key hash, 2^lp of them (8 … 10);
// temporaries in the temp arena; *used says whether out_* hold the result
int ah_encode_partitioned_try(ah_ctx* ctx, const uint64_t* keys, const uint8_t* valid, int64_t off, int64_t n, int encode_nulls, int lp, int slots,
                              int32_t* out_ids, uint64_t* out_dict, int64_t* out_first_rows, int64_t* out_ndict, int32_t* out_null_id, int* used);
// internal (ah_hash.hip): the dense first-seen group ids of 8-byte keys for the id-based aggregates of ah_hash_agg.hip — dictionary_encode with
// nulls encoded (the null key is a group) on the global-table path only (the partition-first encode would take the temp arena the caller's ids live in)
int ah_encode_u64_groups(ah_ctx* ctx, const uint64_t* keys, const uint8_t* kvalid, int64_t koff, int64_t n, int32_t* ids, uint64_t* out_keys,
                         int64_t* out_first_rows, int64_t* out_ngroups, int32_t* out_null_group);
// internal (ah_hash.hip): the dense first-seen ids and first rows of ah_group_ids (ah_group_keys.hip) — over one column of 8-byte words (a
// null is a group; every route of the encode, partition-first included: the caller holds nothing in the scratch or temp arena) and
// over a checked tuple of 2 … 8 columns (the global table with the TupleKeys policy)
int ah_encode_u64_first_seen(ah_ctx* ctx, const uint64_t* keys, const uint8_t* valid, int64_t off, int64_t n, int32_t* ids, int64_t* out_first_rows,
                             int64_t* out_ngroups);
int ah_encode_tuple_first_seen(ah_ctx* ctx, int ncols, const ah_group_key* keys, int64_t n, int32_t* ids, int64_t* out_first_rows, int64_t* out_ngroups);
// … and by two cuts, 64 parents × 2^(lp − 6) partitions (lp = 11 … 13) with LDS tables of `slots` = 4096 or 8192 entries
// distinct valid keys among the first `rows` (≤ 2^16) rows, counted exactly without a table in HBM (ah_hash_part.hip): one launch, one polled wait
int ah_encode_first_look(ah_ctx* ctx, const uint64_t* keys, const uint8_t* valid, int64_t off, int64_t rows, uint64_t* distinct);
int ah_encode_partitioned2_try(ah_ctx* ctx, const uint64_t* keys, const uint8_t* valid, int64_t off, int64_t n, int encode_nulls, int lp, int slots,
                               int32_t* out_ids, uint64_t* out_dict, int64_t* out_first_rows, int64_t* out_ndict, int32_t* out_null_id, int* used);
// internal (ah_ctx.hip): 1..7 device words (8 bytes each, written by work already on the compute stream) → host, through the polled
// mailbox — a cheaper "I need this number before I go on" than a copy + stream synchronisation.  Everything enqueued before it has
// completed when it returns, like a synchronisation of the stream up to that point.
int ah_compact_u64_by_bits(ah_ctx* ctx, const uint64_t* values, const uint8_t* bits, int64_t n, uint64_t* out_values, int64_t* out_rows);   // ah_filter.hip
int ah_check_stall(ah_ctx* ctx);   // AH_EHIP if a kernel reported a stalled look-back since the last check (ah_ctx.hip)
int ah_mailbox_read(ah_ctx* ctx, const unsigned long long* dev_words, int nwords, unsigned long long* out_host);
int ah_mailbox_begin(ah_ctx* ctx, unsigned long long** mb_out, unsigned long long* seq_out);
int ah_mailbox_wait(ah_ctx* ctx, unsigned long long seq, int nwords, unsigned long long* out_host);
#if defined(__HIPCC__)
// ONE thread of a kernel, after everything it reports is final (and visible to it): ≤ 7 words, then the sequence number
__device__ __forceinline__ void ah_mailbox_post(unsigned long long* mb, unsigned long long seq, const unsigned long long* words, int nwords) {
  for (int i = 0; i < nwords; i++) __hip_atomic_store(&mb[i], words[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(&mb[7], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
#endif
int ah_mailbox_read2(ah_ctx* ctx, const unsigned long long* dev_words, int nwords, const unsigned long long* dev_words2, int nwords2,
                     unsigned long long* out_host);
// Grow-only scratch arena. Contents are undefined after the call.
int ah_scratch_reserve(ah_ctx* ctx, size_t nbytes, void** out);
// A second grow-only arena for entry points that call a scratch user (the scan) while their own temporaries are
// live: sort, group-by, var-length take.  One reservation per top-level call, carved by the caller; the block is
// reused by the next call in stream order (no hipMalloc / hipFree — each maps and unmaps the whole range — per call).
// *out_of_memory (nullable) tells a failed hipMalloc — the one failure a caller may answer with a path that needs less — from a failed
// synchronisation or hipFree, which is the caller's to return.
int ah_temp_reserve(ah_ctx* ctx, size_t nbytes, void** out, bool* out_of_memory = nullptr);
// A third grow-only block for ONE temporary that must outlive a whole encode: the packed key column of ah_group_ids.  The encode it
// is handed to takes the scratch arena for its table and — on the partition-first route — the temp arena for its cut, and either
// reservation may grow, which frees the old block: a column carved from one of them could be gone before it is read.
int ah_pack_reserve(ah_ctx* ctx, size_t nbytes, void** out);
// The carving of such a block: every piece starts on a 256-byte boundary.  A caller describes its pieces once (a function of a
// TempCarver&), runs the description on a carver without a base to measure (take only advances `used`), reserves `used` and runs it
// again on the block.
static inline constexpr size_t ah_pad(size_t b) { return (b + 255) & ~(size_t)255; }
struct TempCarver {
  uint8_t* base = nullptr;
  size_t used = 0;
  uint8_t* take(size_t b) { uint8_t* q = base ? base + used : nullptr; used += ah_pad(b); return q; }
  template <typename T> size_t take(T*& p, size_t count) { p = (T*)take(count * sizeof(T)); return ah_pad(count * sizeof(T)); }   // → the piece's bytes
};
// The words of dscalars (ah_ctx: kDsScalars scalar words, then the popcount's partials area) the streaming reductions own.
constexpr int kDsScalars = 64;
constexpr int kDsSum = 0;                           // ah_sum_*, ah_count_set_bits: the one result word
constexpr int kDsFusedSum = 8, kDsFusedCount = 9;   // cmp_filter_sum_*: {sum, count}, read home as two mailbox words
constexpr int kDsMinMax = 12;                       // min_max: {lo, hi}, ≤ 16 bytes
// Owners of the other words: 1–3 filter / take / var-length, 4–8 ah_hash.hip, 9–15 scan / cast / expression flags, 20–23 and 28–29
// ah_groupby.hip, 26–27 ah_sort_msd.hip, 30–36 ah_hash_part.hip, 40–45 ah_comm.hip.
constexpr int kDsGbDone = 20;                       // partition-first group-by: workgroups of gd_finish_kernel that are through, then …
constexpr int kDsGbFlags = 21, kDsGbTotal = 22, kDsGbNullId = 23;   // … {flags (ah_partition.h: kPart*), groups, null group}: read home as three words
constexpr int kDsGbRange = 28;                      // … and [28], [29] the value range of the call (ah_hashing.h)
constexpr int kDsEncFlags = 30, kDsEncTotal = 31, kDsEncNullId = 32;   // partition-first encode: the same three words
constexpr int kDsEncLook = 33, kDsEncLookDone = 34;                 // ah_encode_first_look: the count, the workgroups that have finished
constexpr int kDsEncLargest = 35, kDsEncLargestDone = 36;           // two-cut encode: the largest partition (ms_offs2_kernel), its parents done
constexpr int kDsPopcountPartials = kDsScalars;     // popcount: one word per workgroup …
constexpr int kPopcountMaxPartials = 4096;          // … and as many workgroups at the most
// internal (ah_bitmap.hip): popcount of bits [off, off+nbits) into *total_dev (8 bytes,
// device), enqueued on the compute stream; uses dscalars[kDsPopcountPartials ..] as partials — no scratch.
int ah_popcount_async(ah_ctx* ctx, const uint8_t* bits, int64_t off, int64_t nbits, unsigned long long* total_dev);
int ah_popcount_post(ah_ctx* ctx, const uint8_t* bits, int64_t off, int64_t nbits, unsigned long long* total_dev, const unsigned long long* extra_dev,
                     unsigned long long* out_host /* [2]: *extra_dev, the count */);
// zero a device byte range with one launch on the context's stream (any alignment)
int ah_zero_bytes(ah_ctx* ctx, void* dptr, size_t nbytes);

static inline int ah_type_width(int type) {
  switch (type) {
    case AH_UINT8: case AH_INT8: return 1;
    case AH_UINT16: case AH_INT16: return 2;
    case AH_UINT32: case AH_INT32: case AH_FLOAT32: return 4;
    case AH_UINT64: case AH_INT64: case AH_FLOAT64: return 8;
  }
  return 0;
}

static inline int64_t ah_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

template <typename T> struct TypeTag { using type = T; };
// numeric type id → f(TypeTag<T>{}); false (and no call) for any other id — what that means is the call site's decision
template <class F>
inline bool with_numeric_type(int type, F&& f) {
  switch (type) {
    case AH_UINT8: f(TypeTag<uint8_t>{}); return true;
    case AH_INT8: f(TypeTag<int8_t>{}); return true;
    case AH_UINT16: f(TypeTag<uint16_t>{}); return true;
    case AH_INT16: f(TypeTag<int16_t>{}); return true;
    case AH_UINT32: f(TypeTag<uint32_t>{}); return true;
    case AH_INT32: f(TypeTag<int32_t>{}); return true;
    case AH_UINT64: f(TypeTag<uint64_t>{}); return true;
    case AH_INT64: f(TypeTag<int64_t>{}); return true;
    case AH_FLOAT32: f(TypeTag<float>{}); return true;
    case AH_FLOAT64: f(TypeTag<double>{}); return true;
  }
  return false;
}
// … with a signed integer type as the unsigned type of its width: the carrier of the wrapping kernels
template <class F>
inline bool with_numeric_carrier(int type, F&& f) {
  return with_numeric_type(type, [&](auto t) {
    using T = typename decltype(t)::type;
    if constexpr (__is_floating_point(T)) f(t);
    else f(TypeTag<typename std::make_unsigned<T>::type>{});
  });
}

// The error flag word of a kernel that can fail (bits: ah_elementwise.h), a word of dscalars: cleared on the stream before the
// launch, and brought home after it — a copy to pinned memory and a synchronisation of the stream.
static inline int ah_flag_clear(ah_ctx* c, unsigned* flag) {
  AH_HIP(c, hipMemsetAsync(flag, 0, sizeof(unsigned), c->stream));
  return AH_OK;
}
static inline int ah_flag_read(ah_ctx* c, const unsigned* flag, unsigned* bits) {
  AH_HIP(c, hipMemcpyAsync(c->pinned, flag, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipStreamSynchronize(c->stream));
  *bits = *(volatile unsigned*)c->pinned;
  return AH_OK;
}
int ah_error_of_flag(ah_ctx* ctx, unsigned bits);   // ah_arith_ext.hip: those bits as the reference's error, AH_OK for none

// ---- device helpers ------------------------------------------------------------
#define AH_WAVE 64

// 16-byte vector with only element alignment: lets the backend emit
// global_load_dwordx4 on buffers that are merely element-aligned (Arrow slices:
// &values[offset]); gfx950 runs in unaligned-access mode for global memory.
template <typename T>
struct alignas(sizeof(T)) ah_vec16 {
  T v[16 / sizeof(T)];
};

// 16 bytes at ELEMENT alignment with a nontemporal hint.  Through a native vector type and element-wise moves: a __builtin_bit_cast
// of the loaded vector to the carrier struct compiles to a plain load (seen in the ISA of the first clustered-take kernel), and so
// does a run-time choice between a hinted and a plain access of one address — make the hint a template parameter.
template <typename T>
using ah_raw16 __attribute__((aligned(sizeof(T)))) = T __attribute__((ext_vector_type(16 / sizeof(T))));
template <typename T>
__device__ __forceinline__ ah_vec16<T> ah_ld16_nt(const T* p) {
  const ah_raw16<T> raw = __builtin_nontemporal_load(reinterpret_cast<const ah_raw16<T>*>(p));
  ah_vec16<T> r;
#pragma unroll
  for (int j = 0; j < (int)(16 / sizeof(T)); j++) r.v[j] = raw[j];
  return r;
}
template <typename T>
__device__ __forceinline__ void ah_st16_nt(T* p, const ah_vec16<T>& x) {
  ah_raw16<T> raw;
#pragma unroll
  for (int j = 0; j < (int)(16 / sizeof(T)); j++) raw[j] = x.v[j];
  __builtin_nontemporal_store(raw, reinterpret_cast<ah_raw16<T>*>(p));
}

// the same without the hint: what an element-aligned Arrow slice is read and written with.  `*(const ah_vec16<T>*)p` compiles to
// 2 × 8 bytes (T = 8 bytes), 12 + 4 (4 bytes), 12 + 2 + 1 + 1 (1 byte) — the struct's alignment is its element's — where one
// 16-byte access through the native vector type is legal on gfx950 (unaligned-access mode) and is what the memory pipeline wants.
template <typename T>
__device__ __forceinline__ ah_vec16<T> ah_ld16(const T* p) {
  const ah_raw16<T> raw = *reinterpret_cast<const ah_raw16<T>*>(p);
  ah_vec16<T> r;
#pragma unroll
  for (int j = 0; j < (int)(16 / sizeof(T)); j++) r.v[j] = raw[j];
  return r;
}
template <typename T>
__device__ __forceinline__ void ah_st16(T* p, const ah_vec16<T>& x) {
  ah_raw16<T> raw;
#pragma unroll
  for (int j = 0; j < (int)(16 / sizeof(T)); j++) raw[j] = x.v[j];
  *reinterpret_cast<ah_raw16<T>*>(p) = raw;
}

// Vector i of a column as the validity-aware kernels take it (ah_arith_ext.hip): 16-byte aligned operands stream through
// nontemporal vector accesses (+10–15 % on this chip); element-aligned Arrow slices fall back to the 16-byte
// struct access.  `aligned` is wave-uniform.
template <typename T>
using ah_aligned16 = T __attribute__((ext_vector_type(16 / sizeof(T))));
template <typename ST>
__device__ __forceinline__ ah_vec16<ST> ah_load16(const ST* base, int64_t i, bool aligned) {
  ah_vec16<ST> v;
  if (aligned) {
    const ah_aligned16<ST> t = __builtin_nontemporal_load((const ah_aligned16<ST>*)base + i);
    __builtin_memcpy(&v, &t, 16);
  } else {
    v = ah_ld16<ST>(base + i * (int64_t)(16 / sizeof(ST)));
  }
  return v;
}
template <typename ST>
__device__ __forceinline__ void ah_store16(ST* base, int64_t i, const ah_vec16<ST>& v, bool aligned) {
  if (aligned) {
    ah_aligned16<ST> t;
    __builtin_memcpy(&t, &v, 16);
    __builtin_nontemporal_store(t, (ah_aligned16<ST>*)base + i);
  } else {
    ah_st16<ST>(base + i * (int64_t)(16 / sizeof(ST)), v);
  }
}

// the wave's sum / largest value, valid in lane 0 (the o = 32 … 1 tree); ah_wave_max2: two maxima side by side
template <typename T>
__device__ __forceinline__ T ah_wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
template <typename T>
__device__ __forceinline__ T ah_wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T t = __shfl_down(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
template <typename A, typename B>
__device__ __forceinline__ void ah_wave_max2(A& a, B& b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const A ta = __shfl_down(a, o, 64);
    const B tb = __shfl_down(b, o, 64);
    a = ta > a ? ta : a;
    b = tb > b ? tb : b;
  }
}

__device__ __forceinline__ int ah_lane() { return (int)(threadIdx.x & 63); }

// Read bit i (LSB-first) of a bitmap; NULL bitmap = all ones.
__device__ __forceinline__ int ah_bit(const uint8_t* __restrict__ bm, int64_t i) {
  return bm == nullptr ? 1 : (bm[i >> 3] >> (i & 7)) & 1;
}

// 64 consecutive bits of a bitmap starting at absolute bit position `pos`
// (any alignment), reading only whole 8-byte-aligned words that contain at least
// one bit in [pos, pos + nvalid) — never touches a word outside the caller's
// range, so it cannot fault on the last page of an allocation.  Bits past nvalid
// are returned as 0.  NULL bitmap → all ones (masked to nvalid).
__device__ __forceinline__ uint64_t ah_load_bits64(const uint8_t* __restrict__ bm, int64_t pos, int nvalid);
// The validity word of the 64 consecutive rows a wave is looking at (row `pos0` = the wave's lane 0, the same in every lane):
// the position is moved to scalar registers, so the two 8-byte loads are scalar loads — one per wave instead of a byte load
// (a vector memory instruction with its address arithmetic) per lane and row.
__device__ __forceinline__ uint64_t ah_wave_bits64(const uint8_t* __restrict__ bm, int64_t pos0, int64_t nrows_left) {
  const int64_t p = ((int64_t)__builtin_amdgcn_readfirstlane((int)(pos0 >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)pos0);
  const int64_t left = ((int64_t)__builtin_amdgcn_readfirstlane((int)(nrows_left >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)nrows_left);
  return ah_load_bits64(bm, p, left >= 64 ? 64 : (int)(left < 0 ? 0 : left));
}
__device__ __forceinline__ uint64_t ah_load_bits64(const uint8_t* __restrict__ bm, int64_t pos, int nvalid) {
  uint64_t mask = nvalid >= 64 ? ~0ull : ((1ull << nvalid) - 1);
  if (nvalid <= 0) return 0;
  if (bm == nullptr) return mask;
  uintptr_t addr = (uintptr_t)bm + (uintptr_t)(pos >> 3);
  uintptr_t base = addr & ~(uintptr_t)7;
  int shift = (int)((addr - base) * 8 + (pos & 7));  // 0..63
  const uint64_t* w = (const uint64_t*)base;
  uint64_t lo = w[0] >> shift;
  if (shift != 0 && shift + nvalid > 64) lo |= w[1] << (64 - shift);
  return lo & mask;
}

// Bits [pos, pos + cnt) of a bitmap := the low cnt bits of `word`, every other bit preserved.  A whole aligned word is one
// store; a general position is up to three aligned 32-bit words, atomics because a neighbouring chunk may own the other
// bits of the same word.
__device__ __forceinline__ void put_bits(uint8_t* __restrict__ bm, int64_t pos, unsigned long long word, int cnt) {
  const uintptr_t addr = (uintptr_t)bm + (uintptr_t)(pos >> 3);
  const int sub = (int)(pos & 7);
  if (cnt == 64 && sub == 0 && (addr & 7) == 0) {
    *(unsigned long long*)addr = word;
    return;
  }
  const uintptr_t base = addr & ~(uintptr_t)3;
  int shift = (int)((addr - base) * 8) + sub;  // 0..31
  const unsigned long long m = cnt >= 64 ? ~0ull : ((1ull << cnt) - 1);
  word &= m;
  unsigned* w = (unsigned*)base;
  // 96-bit window
  const unsigned long long mlo = m << shift, vlo = word << shift;
  const unsigned long long mhi = shift ? (m >> (64 - shift)) : 0ull, vhi = shift ? (word >> (64 - shift)) : 0ull;
  const unsigned m0 = (unsigned)mlo, m1 = (unsigned)(mlo >> 32), m2 = (unsigned)mhi;
  const unsigned v0 = (unsigned)vlo, v1 = (unsigned)(vlo >> 32), v2 = (unsigned)vhi;
  if (m0) { atomicAnd(&w[0], ~m0); if (v0) atomicOr(&w[0], v0); }
  if (m1) { atomicAnd(&w[1], ~m1); if (v1) atomicOr(&w[1], v1); }
  if (m2) { atomicAnd(&w[2], ~m2); if (v2) atomicOr(&w[2], v2); }
}

// The ballot of 64-row chunk `chunk` (cnt ≤ 64 rows) into bits out_off + 64·chunk … of `out`: one 64-bit store when the
// output is word-aligned (aligned: out_off % 64 == 0 and `out` 8-byte aligned) and the chunk is full, else put_bits.
__device__ __forceinline__ void put_word(uint8_t* __restrict__ out, int64_t out_off, int aligned, int64_t chunk, unsigned long long word, int cnt) {
  if (aligned && cnt == 64) *(unsigned long long*)(out + (out_off + chunk * 64) / 8) = word;
  else put_bits(out, out_off + chunk * 64, word, cnt);
}

// The ballot of 64-row chunk `chunk` of a column of n rows into a bitmap that starts at row 0 (the output of a kernel that owns
// whole chunks): the chunk's eight bytes, at the column's tail only those that hold a row.
__device__ __forceinline__ void put_chunk_bytes(uint8_t* __restrict__ bm, int64_t chunk, int64_t n, unsigned long long word) {
  const int64_t left = n - chunk * 64;
  const int nbytes = left >= 64 ? 8 : (int)((left + 7) >> 3);
  for (int b = 0; b < nbytes; b++) bm[chunk * 8 + b] = (uint8_t)(word >> (8 * b));
}
