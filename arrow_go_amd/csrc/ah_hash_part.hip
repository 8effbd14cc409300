// ah_hash_part.hip — partition-first unique / dictionary_encode for 8-byte keys: the path for the cardinalities where the one
// global table of ah_hash.hip is neither in LDS nor in L2 (≈ 4·10^5 … 5·10^6 distinct keys).
//
// Replaces (same results, other order of work): doAppendNumeric[uint64] over hashing.Table[uint64].InsertOrGet
// (kernels/vector_hash.go:359-385, internal/hashing/xxh3_memo_table_types.go:283-294), dictionaryEncodeAction
// (vector_hash.go:145-241) and uniqueFinalize (:721-741): ids = order of first occurrence, the null key (if encoded) takes the
// id at which it is first seen (:231-238), a masked null row gets index 0 (vector_hash.go:169-172).
//
// Why.  With 2^20 keys the global table is 32 MiB: every row's probe is a random 64-byte line from the Infinity Cache or HBM,
// and the ids come from a second walk of the same table — PMC showed 92 B/row at 2^20 keys and 237 at 2^24 for 12 algorithmic
// (profiles/r02_pmc_by_workload.json), all of it random lines at the ≈ 50 G/s this chip serves them.  The group-by of
// ah_groupby.hip already avoids that by cutting the rows by key hash first; this file does the same for the encode, whose
// extra difficulty is that it owes an id to every ROW, in row order:
//
//   1 hist, offsets     per (4096-row tile, partition) counts → where every tile's run of every partition starts   (ah_partition.h, ah_bins.h)
//   2 scatter           {key, row | null flag} staged in partition order in LDS, written as runs (20 B/row moved)
//   3 table             ONE workgroup per partition: its keys in an 8192-slot open-addressing table in LDS {key, first row};
//                       every record learns its SLOT (2 bytes, partition order); the table and the first-row bits leave
//   4 rank              first rows → n-bit bitmap → prefix popcount = the sequential memo index (the argument of ah_hash.hip);
//                       every used slot gets its id, dict[id] = key
//   5 resolve           one workgroup per partition again, the partition's slot → id table in LDS: slot numbers → ids, still
//                       in partition order (6 B/row)
//   6 unpermute         per tile: its runs are read back (id + row), placed at row-in-tile in LDS, 4096 ids leave coalesced
//                       (the way the binned Take sends gathered values home, ah_take_binned.hip)
// `unique` (no ids wanted) stops after step 4.  Everything is streaming or ≥ 64-byte runs: 8 + 20 + 14 + 6 + 12 = 60 B/row.
// Nothing depends on timing: a slot number is arbitrary, an id is a function of first rows only — the bytes are those of the
// global-table path (tests/test_gpu_parity.py::test_hash_encode_partitioned).
//
// One workgroup per partition needs partitions of similar size: a key that owns a large share of the rows (Zipf) makes one
// partition many times the others — seen on the host right after the offsets pass, and such columns stay on the other path.
#include <vector>
#include "ah_common.h"
#include "ah_hashing.h"
#include "ah_bins.h"
#include "ah_part_driver.h"
#include "ah_msd.h"

namespace {

// LDS table of one partition: S slots (open addressing, aligned groups of 4) + the all-ones key (slot S) and the null key (S + 1);
// ¾ S keys admitted — beyond that the attempt is void (the estimate was far off); a partition's slice of the global copies is
// S + 8 entries.  S = 8192 (96 KiB: one workgroup per CU) for the one-cut path; S = 4096 for the two-cut path, whose partitions
// hold only ≈ 8 Ki rows: three workgroups per CU hide each other's LDS round trips, and a table costs half as much to set up and dump.
constexpr int kESlots = 8192, kESlots2 = 4096;
constexpr unsigned short kMaskedSlot = 0xFFFFu;   // a null row whose nulls are not encoded: index 0, no dictionary entry

template <int S>
__device__ __forceinline__ unsigned enc_group(unsigned long long key) {   // first slot group; inside a partition the keys agree in the top bits of gb_mix
  return ((((unsigned)key * 0x9E3779B1u) ^ ((unsigned)(key >> 32) * 0x85EBCA6Bu)) >> 18) & (unsigned)(S - 4);
}

// ---- 3: one workgroup per partition ------------------------------------------------------------------------------------------
template <int S, bool BATCH>
__global__ __launch_bounds__(kThreads) void enc_table_kernel(const unsigned long long* __restrict__ pkeys, const unsigned* __restrict__ prows,
                                                              const unsigned* __restrict__ binstart, int encode_nulls,
                                                              unsigned long long* __restrict__ tab_key, unsigned* __restrict__ tab_first,
                                                              unsigned short* __restrict__ rec_slot, unsigned long long* __restrict__ firsts,
                                                              unsigned* __restrict__ overflow, uint8_t* __restrict__ fbytes = nullptr) {
  constexpr int kLS = S + 2, kStride = S + 8, kSoft = S / 4 * 3;
  __shared__ __attribute__((aligned(16))) unsigned long long l_key[kLS];
  __shared__ unsigned l_first[kLS];
  __shared__ unsigned s_used;
  const int t = threadIdx.x, part = blockIdx.x;
  const int64_t r0 = binstart[part], r1 = binstart[part + 1];
  for (int j = t; j < kLS; j += kThreads) { l_key[j] = kEmpty; l_first[j] = kNoRow; }
  if (t == 0) s_used = 0;
  __syncthreads();
  const unsigned lkey_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned long long*)l_key;   // LDS byte address of the key table
  // find or claim the slot of `key` (−1: the table is full)
  auto slot_of = [&](unsigned long long key) -> int {
    unsigned g = enc_group<S>(key);
    for (;;) {
      // two ds_read_b128, spelled out (the compiler would split them into ds_read2_b64: half the banks per access, ah_groupby.hip)
      typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
      u64x2 a, c;
      asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)"
                   : "=&v"(a), "=&v"(c) : "v"(lkey_base + g * 8u) : "memory");
      const bool h0 = a.x == key, h1 = a.y == key, h2 = c.x == key, h3 = c.y == key;
      const bool e0 = a.x == kEmpty, e1 = a.y == kEmpty, e2 = c.x == kEmpty, e3 = c.y == kEmpty;
      const bool y0 = h0 || e0, y1 = h1 || e1, y2 = h2 || e2, y3 = h3 || e3;
      if (!(y0 || y1 || y2 || y3)) { g = (g + 4) & (S - 1); continue; }
      const int j = (int)g + (y0 ? 0 : y1 ? 1 : y2 ? 2 : 3);
      if (h0 || (!e0 && (h1 || (!e1 && (h2 || (!e2 && h3)))))) return j;   // the key sits in front of the first empty slot
      if (atomicAdd(&s_used, 1u) >= (unsigned)kSoft) return -1;             // tickets are never returned: "full" sticks
      const unsigned long long cur = atomicCAS(&l_key[j], kEmpty, key);
      if (cur == kEmpty || cur == key) return j;
      // another key took it meanwhile: look at the group again
    }
  };
  constexpr int U = 4;
  constexpr int64_t kStep = (int64_t)kThreads * U;
  unsigned long long nk[U];
  unsigned nrw[U];
  auto load_step = [&](int64_t b) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = b + u * kThreads + t;
      const bool in = i < r1;
      nk[u] = in ? __builtin_nontemporal_load(&pkeys[i]) : 0ull;
      nrw[u] = in ? __builtin_nontemporal_load(&prows[i]) : 0u;
    }
  };
  bool full = false;
  // the lane's previous row: a key that owns much of the partition would put every lane on one slot group
  unsigned long long p_key = 0;
  int p_slot = -2;
  if (r0 < r1) load_step(r0);
  __builtin_amdgcn_s_waitcnt(0);   // enter the loop with nothing pending: see gb_aggregate_kernel on the compiler's wait counts
  for (int64_t b = r0; b < r1; b += kStep) {
    unsigned long long k[U];
    unsigned rw[U];
#pragma unroll
    for (int u = 0; u < U; u++) { k[u] = nk[u]; rw[u] = nrw[u]; }
    if (b + kStep < r1) load_step(b + kStep);
    if constexpr (BATCH) {
    // Most records find their key where the table already has it (a partition holds ~4096 keys and 64 × as many records), so the
    // U records' first slot groups are read TOGETHER — 2 U ds_read_b128 in flight, one wait — and only a record whose key is not
    // in front of the first empty slot of its group (a new key, or a probe sequence that goes on) takes the serial find-or-claim
    // loop.  One record at a time, the pass spent half its wave cycles parked on LDS round trips (4 waves per SIMD: a partition
    // is one workgroup, 256 partitions one workgroup per CU).
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    unsigned g[U];
    u64x2 qa[U], qc[U];
#pragma unroll
    for (int u = 0; u < U; u++) g[u] = enc_group<S>(k[u]);
    static_assert(U == 4, "the batched probe below is written for four records");
    asm volatile(
        "ds_read_b128 %0, %8\n\tds_read_b128 %1, %8 offset:16\n\t"
        "ds_read_b128 %2, %9\n\tds_read_b128 %3, %9 offset:16\n\t"
        "ds_read_b128 %4, %10\n\tds_read_b128 %5, %10 offset:16\n\t"
        "ds_read_b128 %6, %11\n\tds_read_b128 %7, %11 offset:16\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(qa[0]), "=&v"(qc[0]), "=&v"(qa[1]), "=&v"(qc[1]), "=&v"(qa[2]), "=&v"(qc[2]), "=&v"(qa[3]), "=&v"(qc[3])
        : "v"(lkey_base + g[0] * 8u), "v"(lkey_base + g[1] * 8u), "v"(lkey_base + g[2] * 8u), "v"(lkey_base + g[3] * 8u)
        : "memory");
    int js[U];
    unsigned rows[U];
    unsigned pend = 0;
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = b + u * kThreads + t;
      rows[u] = rw[u] & kRowMask;
      int j = -3;   // −3: not a record of this partition
      if (i < r1) {
        const unsigned long long key = k[u];
        if (rw[u] & kKeyNull) j = encode_nulls ? S + 1 : -2;
        else if (key == kEmpty) j = S;
        else if (p_slot >= 0 && p_key == key) j = p_slot;
        else {
          const bool h0 = qa[u].x == key, h1 = qa[u].y == key, h2 = qc[u].x == key, h3 = qc[u].y == key;
          const bool e0 = qa[u].x == kEmpty, e1 = qa[u].y == kEmpty, e2 = qc[u].x == kEmpty;
          if (h0 || (!e0 && (h1 || (!e1 && (h2 || (!e2 && h3)))))) j = (int)g[u] + (h0 ? 0 : h1 ? 1 : h2 ? 2 : 3);
          else { j = -4; pend |= 1u << u; }   // −4: to the find-or-claim loop below
          p_key = key; p_slot = j;            // (a pending slot is negative: the next record does not reuse it)
        }
      }
      js[u] = j;
    }
    // the stragglers of all U records in ONE divergent phase: some lane of a wave always has one (a twentieth of the records × 64
    // lanes), so a per-record fallback would run the serial loop for every record after all
    while (pend) {
      const int u = __builtin_ctz(pend);
      pend &= pend - 1;
      const unsigned long long key = u == 0 ? k[0] : u == 1 ? k[1] : u == 2 ? k[2] : k[3];
      const int j = slot_of(key);
      if (u == 0) js[0] = j; else if (u == 1) js[1] = j; else if (u == 2) js[2] = j; else js[3] = j;
      if (key == p_key) p_slot = j;
    }
    unsigned fr[U];
#pragma unroll
    for (int u = 0; u < U; u++) fr[u] = js[u] >= 0 ? l_first[js[u]] : 0u;
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = b + u * kThreads + t;
      const int j = js[u];
      if (j >= 0) {
        if (fr[u] > rows[u]) atomicMin(&l_first[j], rows[u]);   // rows of a key arrive mostly in ascending order: a read is half an atomic
      } else if (j == -1) {
        full = true;
      }
      if (rec_slot && j != -3) rec_slot[i] = j >= 0 ? (unsigned short)j : kMaskedSlot;
    }
    } else {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = b + u * kThreads + t;
      if (i >= r1) continue;
      const unsigned row = rw[u] & kRowMask;
      int j;
      if (rw[u] & kKeyNull) j = encode_nulls ? S + 1 : -2;
      else if (k[u] == kEmpty) j = S;
      else if (p_slot >= 0 && p_key == k[u]) j = p_slot;
      else { j = slot_of(k[u]); p_key = k[u]; p_slot = j; }
      if (j >= 0) {
        if (l_first[j] > row) atomicMin(&l_first[j], row);   // rows of a key arrive mostly in ascending order: a read is half an atomic
      } else if (j == -1) {
        full = true;
      }
      if (rec_slot) rec_slot[i] = j >= 0 ? (unsigned short)j : kMaskedSlot;
    }
    }
  }
  if (full) atomicExch(overflow, 1u);
  __syncthreads();
  const int64_t gbase = (int64_t)part * kStride;
  for (int j = t; j < kStride; j += kThreads) {
    const unsigned fr = j < kLS ? l_first[j] : kNoRow;
    if (j < kLS && tab_key) tab_key[gbase + j] = l_key[j];   // (not wanted when the dictionary is compacted from the column)
    tab_first[gbase + j] = fr;
    if (fr != kNoRow) {
      if (fbytes) fbytes[fr] = 1;   // a plain byte store into the byte map (enc_bytes_to_bits_kernel packs it): no device-scope read-modify-write per key
      else atomicOr(&firsts[fr >> 6], 1ull << (fr & 63));
    }
  }
}

// byte map (one byte per row, 1 = a first occurrence) → the bitmap: a lane packs 64 bytes into one word
__global__ __launch_bounds__(kBlock) void enc_bytes_to_bits_kernel(const uint8_t* __restrict__ fbytes, int64_t nwords, unsigned long long* __restrict__ firsts) {
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= nwords) return;
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  const u64x2* src = reinterpret_cast<const u64x2*>(fbytes + w * 64);
  unsigned long long bits = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const u64x2 v = __builtin_nontemporal_load(src + q);
#pragma unroll
    for (int h = 0; h < 2; h++) {
      // eight bytes of 0 / 1 → eight bits: the bytes' low bits gathered by a multiply (0x0102040810204080 puts byte k's bit at position 56 + k)
      const unsigned long long x = (h ? v.y : v.x) & 0x0101010101010101ull;
      bits |= ((x * 0x0102040810204080ull) >> 56) << (q * 16 + h * 8);
    }
  }
  firsts[w] = bits;
}

// ---- 4: ids of the used slots (tab_first is overwritten with them), the dictionary -----------------------------------------------
__global__ __launch_bounds__(kBlock) void enc_assign_kernel(const unsigned long long* __restrict__ tab_key, unsigned* __restrict__ tab_first, int64_t nslots,
                                                             const unsigned long long* __restrict__ firsts, const unsigned* __restrict__ wordprefix,
                                                             const int64_t* __restrict__ tileoff, unsigned long long* __restrict__ dict,
                                                             long long* __restrict__ first_rows, int* __restrict__ null_id, int slots,
                                                             const ulonglong2* __restrict__ rank_rec) {
  // four slots per lane, their chains (first row → bitmap word, word prefix, tile offset → id → three scattered stores) side by
  // side: one slot per iteration left every wave with a single dependent chain of five round trips (2^24 keys: 1.0 ms for this pass)
  constexpr int U = 4;
  const int64_t stride = (int64_t)gridDim.x * kBlock * U;
  for (int64_t s0 = (int64_t)blockIdx.x * kBlock * U + threadIdx.x; s0 < nslots; s0 += stride) {
    unsigned fr[U], id[U];
    unsigned long long key[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t s = s0 + (int64_t)u * kBlock;
      fr[u] = s < nslots ? tab_first[s] : kNoRow;
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t s = s0 + (int64_t)u * kBlock;
      id[u] = 0; key[u] = 0;
      if (fr[u] != kNoRow) {
        if (rank_rec) {   // {bitmap word, ranks below the word} in ONE 16-byte gather instead of three gathers from three arrays
          const ulonglong2 rr = rank_rec[fr[u] >> 6];
          id[u] = (unsigned)rr.y + (unsigned)__popcll(rr.x & ((1ull << (fr[u] & 63)) - 1));
        } else {
          id[u] = rank_of_row(fr[u], firsts, wordprefix, tileoff);
        }
        if (dict) key[u] = tab_key[s];
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t s = s0 + (int64_t)u * kBlock;
      if (fr[u] == kNoRow) continue;
      tab_first[s] = id[u];
      const int in_part = (int)(s % (slots + 8));
      unsigned long long k = key[u];
      if (in_part == slots) k = kEmpty;
      if (in_part == slots + 1) { k = 0; *null_id = (int)id[u]; }   // GetDictArrayData: the null slot keeps the fresh buffer's zero
      if (dict) dict[id[u]] = k;
      if (first_rows) first_rows[id[u]] = (long long)fr[u];
    }
  }
}

// the null entry: its id (when no assign pass ran: from the null slot of table 0, where all null keys went) and its dictionary value —
// GetDictArrayData leaves the fresh buffer's zero there, whatever bits the first null row holds
__global__ void enc_null_entry_kernel(const unsigned* __restrict__ tab_first, int slots, int need_rank, const unsigned long long* __restrict__ firsts,
                                      const unsigned* __restrict__ wordprefix, const int64_t* __restrict__ tileoff, int* __restrict__ null_id,
                                      unsigned long long* __restrict__ dict) {
  if (need_rank) {
    const unsigned fr = tab_first[slots + 1];
    if (fr != kNoRow) *null_id = (int)rank_of_row(fr, firsts, wordprefix, tileoff);
  }
  const int id = *null_id;
  if (id >= 0 && dict) dict[id] = 0;
}

__global__ __launch_bounds__(kBlock) void rank_rec_kernel(const unsigned long long* __restrict__ firsts, const unsigned* __restrict__ wordprefix,
                                                           const int64_t* __restrict__ tileoff, int64_t nwords, ulonglong2* __restrict__ rec) {
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w < nwords) rec[w] = make_ulonglong2(firsts[w], (unsigned long long)(tileoff[w >> kRankTileLog2] + wordprefix[w]));
}

// ids of the slots + the dictionary (and the first rows) in id order.  compact = false: every used slot writes its key to dict[id] —
// ids follow first rows, so these are scattered 8-byte stores, two per key, behind two scattered reads (2^24 keys: 0.87 ms).
// compact = true: the dictionary is the key column itself compacted by the first-occurrence bitmap (ah_filter.hip: tiles without a
// first occurrence are never fetched, the output leaves as whole lines), and the slots only look their ids up — or nothing at
// all when the caller wants no ids (unique).
int enc_emit(ah_ctx* c, bool compact, bool need_ids, const unsigned long long* tab_key, unsigned* tab_first, int64_t nslots, const unsigned long long* firsts,
             const unsigned* wordprefix, const int64_t* tileoff, const uint64_t* keys, int64_t n, uint64_t* out_dict, int64_t* out_first_rows, int* null_id,
             int slots) {
  const unsigned agrid = ah_stream_grid(c, ah_ceil_div(nslots, (int64_t)kBlock * 4));
  if (!compact) {
    enc_assign_kernel<<<agrid, kBlock, 0, c->stream>>>(tab_key, tab_first, nslots, firsts, wordprefix, tileoff, (unsigned long long*)out_dict,
                                                       (long long*)out_first_rows, null_id, slots, nullptr);
    AH_LAUNCH_CHECK(c);
    return AH_OK;
  }
  int rc = ah_compact_u64_by_bits(c, keys, (const uint8_t*)firsts, n, out_dict, out_first_rows);
  if (rc != AH_OK) return rc;
  if (need_ids) {
    // the key table is not read any more (the dictionary came from the column): its block holds the rank records
    const int64_t nwords = ah_ceil_div(n, 64);
    ulonglong2* rec = nullptr;
    if (nslots * 8 >= nwords * 16) {
      rec = (ulonglong2*)tab_key;
      rank_rec_kernel<<<(unsigned)ah_ceil_div(nwords, kBlock), kBlock, 0, c->stream>>>(firsts, wordprefix, tileoff, nwords, rec);
      AH_LAUNCH_CHECK(c);
    }
    enc_assign_kernel<<<agrid, kBlock, 0, c->stream>>>(tab_key, tab_first, nslots, firsts, wordprefix, tileoff, nullptr, nullptr, null_id, slots, rec);
    AH_LAUNCH_CHECK(c);
  }
  enc_null_entry_kernel<<<1, 1, 0, c->stream>>>(tab_first, slots, need_ids ? 0 : 1, firsts, wordprefix, tileoff, null_id, (unsigned long long*)out_dict);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}

// ---- 5: slot numbers → ids, in partition order ---------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(kThreads) void enc_resolve_kernel(const unsigned short* __restrict__ rec_slot, const unsigned* __restrict__ tab_id,
                                                                const unsigned* __restrict__ binstart, int* __restrict__ rec_id, int split) {
  constexpr int kLS = S + 2, kStride = S + 8;
  __shared__ unsigned l_id[kLS];
  // `split` workgroups share a partition's records (each loads the partition's 32 KiB id table): with one workgroup per
  // partition 256 partitions put 16 waves on a CU and the pass waited on memory 90 % of its time (2.4 TB/s)
  const int t = threadIdx.x, part = blockIdx.x / split, piece = blockIdx.x % split;
  const int64_t p0 = binstart[part], p1 = binstart[part + 1];
  const int64_t per = (((p1 - p0 + split - 1) / split) + 63) & ~(int64_t)63;
  const int64_t r0 = p0 + piece * per, r1 = r0 + per < p1 ? r0 + per : p1;
  if (r0 >= r1) return;
  for (int j = t; j < kLS; j += kThreads) l_id[j] = tab_id[(int64_t)part * kStride + j];
  __syncthreads();
  // Eight records per lane: ONE 16-byte load of slot numbers, two 16-byte stores of ids (2-byte loads moved 128 bytes per wave and
  // instruction: 2.4–3.2 TB/s).  The piece's ragged ends — up to the first and from the last multiple of 8 — go one record per lane.
  auto one = [&](int64_t i) {
    const unsigned short sl = rec_slot[i];
    rec_id[i] = sl == kMaskedSlot ? 0 : (int)l_id[sl];
  };
  const int64_t a0 = (r0 + 7) & ~(int64_t)7, a1 = r1 & ~(int64_t)7;
  if (a0 >= a1) {
    for (int64_t i = r0 + t; i < r1; i += kThreads) one(i);
    return;
  }
  if (r0 + t < a0) one(r0 + t);
  if (a1 + t < r1) one(a1 + t);
  typedef unsigned v4u __attribute__((ext_vector_type(4)));
  typedef int v4i __attribute__((ext_vector_type(4)));
  const int64_t nvec = (a1 - a0) >> 3;
  const v4u* __restrict__ src = reinterpret_cast<const v4u*>(rec_slot + a0);   // a0 is a multiple of 8 records = 16 bytes; the arrays are 256-byte aligned
  v4i* __restrict__ dst = reinterpret_cast<v4i*>(rec_id + a0);
  constexpr int U = 2;
  for (int64_t b = 0; b < nvec; b += (int64_t)kThreads * U) {
    v4u w[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = b + u * kThreads + t;
      w[u] = i < nvec ? __builtin_nontemporal_load(&src[i]) : (v4u){0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = b + u * kThreads + t;
      if (i >= nvec) continue;
      int id[8];
#pragma unroll
      for (int e = 0; e < 8; e++) {
        const unsigned sl = (w[u][e >> 1] >> (16 * (e & 1))) & 0xffffu;
        id[e] = sl == kMaskedSlot ? 0 : (int)l_id[sl];
      }
      __builtin_nontemporal_store((v4i){id[0], id[1], id[2], id[3]}, &dst[2 * i]);
      __builtin_nontemporal_store((v4i){id[4], id[5], id[6], id[7]}, &dst[2 * i + 1]);
    }
  }
}

// ---- 6: ids back to row order, G consecutive tiles per workgroup -------------------------------------------------------------------
// The tile's (group's) runs are found again (tile_bin_offsets, bin_of_staged: ah_bins.h), every record's id is placed at its row in
// LDS, and the ids leave as whole lines.  Inside a partition the runs of consecutive tiles lie one after the other, so a group's
// records of a partition are ONE run G times as long (256 partitions: 16 records = 64 bytes per tile, 256 bytes per group of four —
// with G = 1 the kernel reads 64-byte pieces at 2.3 TB/s).  LDS: G · 16 KiB of ids.
template <int G>
__global__ __launch_bounds__(kThreads) void enc_unpermute_group_kernel(const int* __restrict__ rec_id, const unsigned* __restrict__ prows,
                                                                       const unsigned* __restrict__ cnt_tm, const unsigned* __restrict__ toffs, int nb,
                                                                       int64_t ntiles, int64_t n, int32_t* __restrict__ out_ids) {
  __shared__ unsigned s_cnt[kMaxBins], s_start[kMaxBins], s_goff[kMaxBins], s_wsum[kThreads / 64];
  __shared__ int s_out[G * kGbTile];
  const int64_t grp = xcd_contiguous_tile((ntiles + G - 1) / G);
  if (grp < 0) return;
  const int64_t tile0 = grp * G;
  unsigned excl = 0, cnt = 0;
  if ((int)threadIdx.x < nb) {
    excl = toffs[tile0 * nb + threadIdx.x];
#pragma unroll
    for (int g = 0; g < G; g++)
      if (tile0 + g < ntiles) cnt += cnt_tm[(tile0 + g) * nb + threadIdx.x];
  }
  tile_bin_offsets(cnt, excl, nb, s_cnt, s_start, s_goff, s_wsum);
  const int64_t base = tile0 * kGbTile;
  const int grp_n = n - base >= (int64_t)G * kGbTile ? G * kGbTile : (int)(n - base);
#pragma unroll 1
  for (int c = 0; c < G; c++) {
    int lo[kGbRows];
    bin_of_staged<kGbRows, kMaxBinSteps>(s_start, nb, c * kGbTile, lo);
    int id[kGbRows];
    unsigned rw[kGbRows];
#pragma unroll
    for (int k = 0; k < kGbRows; k++) {
      const int lp = c * kGbTile + k * kThreads + threadIdx.x;
      id[k] = 0; rw[k] = 0;
      if (lp < grp_n) {
        const int64_t e = (int64_t)s_goff[lo[k]] + lp;
        id[k] = __builtin_nontemporal_load(&rec_id[e]);
        rw[k] = __builtin_nontemporal_load(&prows[e]);
      }
    }
#pragma unroll
    for (int k = 0; k < kGbRows; k++)
      if (c * kGbTile + k * kThreads + (int)threadIdx.x < grp_n) s_out[(int64_t)(rw[k] & kRowMask) - base] = id[k];
  }
  __syncthreads();
  store_staged<G * kGbRows>(s_out, grp_n, out_ids, base);
}

void launch_enc_unpermute(ah_ctx* c, const int* rec_id, const unsigned* prows, const unsigned* cnt_tm, const unsigned* toffs, int nb, int64_t ntiles,
                          int64_t n, int32_t* out_ids) {
  const int G = c->opt_encode_unperm_group;
  const int g = G >= 8 ? 8 : (G >= 4 ? 4 : (G >= 2 ? 2 : 1));
  const unsigned grid = (unsigned)(((ah_ceil_div(ntiles, g) + 7) / 8) * 8);
  if (g == 8) enc_unpermute_group_kernel<8><<<grid, kThreads, 0, c->stream>>>(rec_id, prows, cnt_tm, toffs, nb, ntiles, n, out_ids);
  else if (g == 4) enc_unpermute_group_kernel<4><<<grid, kThreads, 0, c->stream>>>(rec_id, prows, cnt_tm, toffs, nb, ntiles, n, out_ids);
  else if (g == 2) enc_unpermute_group_kernel<2><<<grid, kThreads, 0, c->stream>>>(rec_id, prows, cnt_tm, toffs, nb, ntiles, n, out_ids);
  else enc_unpermute_group_kernel<1><<<grid, kThreads, 0, c->stream>>>(rec_id, prows, cnt_tm, toffs, nb, ntiles, n, out_ids);
}


// ---- more than 1024 partitions: a second cut ---------------------------------------------------------------------------------------
// Beyond ≈ 4.5 M keys 1024 LDS tables are not enough, and one scatter into thousands of partitions would write runs of one or two
// rows.  So the cut is made twice, as in the MSD sort and the large group-by (ah_msd.h): level 1 = the pass above with 64
// partitions ("parents"); level 2 cuts every parent into 2^lb2 ≤ 128 partitions — its tiles are "virtual tiles" that never cross
// a parent boundary and all run on one XCD.  A level-2 record is {key, row | flag} plus its position in the virtual tile (2 bytes):
// the ids go home in two steps, virtual tile by virtual tile back into level-1 order, then tile by tile into row order.
__device__ __forceinline__ unsigned e2_digit(unsigned long long key, unsigned rw, int lp, unsigned mask) {
  return (rw & kKeyNull) ? 0u : ((unsigned)(gb_mix(key) >> (64 - lp)) & mask);   // level 1 took the top 6 of these lp bits (null keys: partition 0 of parent 0)
}
struct E2Digit {   // tile_hist_kernel's view of the level-1 records (ah_msd.h)
  static constexpr int kMaxDigits = kThreads;
  const unsigned long long* pkeys; const unsigned* prows; int lp; unsigned mask;
  // (null keys all sit in parent 0: the other 63 parents' histograms read the keys alone, 8 instead of 12 bytes per record)
  __device__ __forceinline__ unsigned digit(int64_t i, int parent) const {
    return e2_digit(__builtin_nontemporal_load(&pkeys[i]), parent == 0 ? __builtin_nontemporal_load(&prows[i]) : 0u, lp, mask);
  }
};

__global__ __launch_bounds__(kThreads) void e2_scatter_kernel(const unsigned long long* __restrict__ pkeys, const unsigned* __restrict__ prows, int64_t n,
                                                               const unsigned* __restrict__ pstart, int nparents, int lp, unsigned mask, int nb,
                                                               const unsigned* __restrict__ toffs, unsigned long long* __restrict__ out_keys,
                                                               unsigned* __restrict__ out_rows, unsigned short* __restrict__ out_j) {
  __shared__ unsigned s_cnt[kThreads], s_start[kThreads], s_goff[kThreads], s_wsum[kThreads / 64];
  __shared__ unsigned s_a[kThreads], s_b[kThreads];
  __shared__ unsigned long long s_stage[kMsTile];
  __shared__ uint16_t s_bin[kMsTile];
  __shared__ int s_pick;
  const TileRange r = ms_tile(pstart, nparents, n, s_a, s_b, s_wsum, &s_pick);
  if (r.parent < 0) return;
  const int t = threadIdx.x;
  s_cnt[t] = 0;
  unsigned long long k[kMsRows];
  unsigned rw[kMsRows], dg[kMsRows], rank[kMsRows];
  bool live[kMsRows];
#pragma unroll
  for (int u = 0; u < kMsRows; u++) {
    const int64_t i = r.lo + u * kThreads + t;
    live[u] = i < r.hi;
    k[u] = live[u] ? __builtin_nontemporal_load(&pkeys[i]) : 0ull;
    rw[u] = live[u] ? __builtin_nontemporal_load(&prows[i]) : 0u;
  }
  unsigned goff_excl = 0;
  if (t < nb) goff_excl = toffs[r.id * nb + t];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kMsRows; u++) {
    dg[u] = e2_digit(k[u], rw[u], lp, mask);
    rank[u] = live[u] ? atomicAdd(&s_cnt[dg[u]], 1u) : 0u;
  }
  __syncthreads();
  block_excl_scan(s_cnt, s_start, s_wsum, nb);   // nb ≤ 128
  if (t < nb) s_goff[t] = goff_excl - s_start[t];
  const int tile_n = (int)(r.hi - r.lo);
#pragma unroll
  for (int u = 0; u < kMsRows; u++)
    if (live[u]) { const unsigned q = s_start[dg[u]] + rank[u]; s_stage[q] = k[u]; s_bin[q] = (uint16_t)dg[u]; }
  __syncthreads();
  int64_t dst[kMsRows];
#pragma unroll
  for (int u = 0; u < kMsRows; u++) {
    const int q = u * kThreads + t;
    dst[u] = q < tile_n ? (int64_t)s_goff[s_bin[q]] + q : -1;
    if (dst[u] >= 0) out_keys[dst[u]] = s_stage[q];
  }
  __syncthreads();
  // second round: {row word, position in the virtual tile} as one 8-byte staged element
#pragma unroll
  for (int u = 0; u < kMsRows; u++)
    if (live[u]) s_stage[s_start[dg[u]] + rank[u]] = ((unsigned long long)(unsigned)(u * kThreads + t) << 32) | rw[u];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kMsRows; u++)
    if (dst[u] >= 0) {
      const unsigned long long x = s_stage[u * kThreads + t];
      out_rows[dst[u]] = (unsigned)x;
      out_j[dst[u]] = (unsigned short)(x >> 32);
    }
}

// ---- ids of the level-2 records → back at their level-1 positions, G consecutive virtual tiles of a parent per workgroup ---------------
// As enc_unpermute_group_kernel does for level 1 (353 → 205 µs there): inside a digit the runs of consecutive virtual tiles lie one
// after the other (ms_offs2_kernel walks the tiles in order), so the group reads ONE run per digit, G times as long (nb2 = 128 digits:
// 32 records per tile).  A record's tile inside the group follows from its offset in the group's run of its digit (s_cum: cumulative
// counts per digit after each of the group's tiles but the last); its 2-byte position is relative to that tile.
// vt0, gt: the group's first virtual tile and how many it has; [lo, lo + group_n): its level-1 positions.  nb ≤ 128.
template <int G>
__device__ __forceinline__ void e2_unpermute_body(const int* __restrict__ rec_id, const unsigned short* __restrict__ rec_j, const unsigned* __restrict__ cnt,
                                                  const unsigned* __restrict__ toffs, int nb, int64_t vt0, int gt, int64_t lo, int group_n, unsigned* s_cnt,
                                                  unsigned* s_start, unsigned* s_goff, unsigned* s_wsum, unsigned (*s_cum)[128], int* s_out,
                                                  int* __restrict__ rec_id1) {
  const int t = threadIdx.x;
  unsigned excl = 0, c = 0;
  if (t < nb) {
    excl = toffs[vt0 * nb + t];
#pragma unroll
    for (int q = 0; q < G; q++) {
      if (q < gt) c += cnt[(vt0 + q) * nb + t];
      if (q < G - 1) s_cum[q][t] = c;
    }
  }
  tile_bin_offsets(c, excl, nb, s_cnt, s_start, s_goff, s_wsum);
#pragma unroll 1
  for (int ch = 0; ch < G; ch++) {
    int dlo[kMsRows];
    bin_of_staged<kMsRows, 8>(s_start, nb, ch * kMsTile, dlo);   // 2^8 ≥ nb
    int id[kMsRows];
    unsigned short jp[kMsRows];
#pragma unroll
    for (int k = 0; k < kMsRows; k++) {
      const int lp = ch * kMsTile + k * kThreads + t;
      id[k] = 0; jp[k] = 0;
      if (lp < group_n) {
        const int64_t e = (int64_t)s_goff[dlo[k]] + lp;
        id[k] = __builtin_nontemporal_load(&rec_id[e]);
        jp[k] = __builtin_nontemporal_load(&rec_j[e]);
      }
    }
#pragma unroll
    for (int k = 0; k < kMsRows; k++) {
      const int lp = ch * kMsTile + k * kThreads + t;
      if (lp < group_n) {
        int tile = 0;
        if (G > 1) {
          const unsigned q = (unsigned)lp - s_start[dlo[k]];   // offset in the group's run of this digit
#pragma unroll
          for (int w = 0; w < G - 1; w++) tile += q >= s_cum[w][dlo[k]] ? 1 : 0;
        }
        s_out[tile * kMsTile + jp[k]] = id[k];
      }
    }
  }
  __syncthreads();
  store_staged<G * kMsRows>(s_out, group_n, rec_id1, lo);
}

// one virtual tile per workgroup (option encode_unperm2_group = 0), picked as the level-2 scatter picks it.  This one keeps the skeleton
// spelled out: over tile_bin_offsets / bin_of_staged (ah_bins.h) it took 27 registers where it has a budget of 25 (tests/test_isa_hints.py)
__global__ __launch_bounds__(kThreads) void e2_unpermute_kernel(const int* __restrict__ rec_id, const unsigned short* __restrict__ rec_j,
                                                                 const unsigned* __restrict__ cnt, const unsigned* __restrict__ toffs, int64_t n,
                                                                 const unsigned* __restrict__ pstart, int nparents, int nb, int* __restrict__ rec_id1) {
  __shared__ unsigned s_cnt[kThreads], s_start[kThreads], s_goff[kThreads], s_wsum[kThreads / 64];
  __shared__ unsigned s_a[kThreads], s_b[kThreads];
  __shared__ int s_out[kMsTile];
  __shared__ int s_pick;
  const TileRange r = ms_tile(pstart, nparents, n, s_a, s_b, s_wsum, &s_pick);
  if (r.parent < 0) return;
  const int t = threadIdx.x;
  unsigned excl = 0;
  s_cnt[t] = 0;
  if (t < nb) { s_cnt[t] = cnt[r.id * nb + t]; excl = toffs[r.id * nb + t]; }
  __syncthreads();
  block_excl_scan(s_cnt, s_start, s_wsum, nb);
  if (t < nb) s_goff[t] = excl - s_start[t];
  __syncthreads();
  const int tile_n = (int)(r.hi - r.lo);
  int lo[kMsRows], hi[kMsRows];
#pragma unroll
  for (int k = 0; k < kMsRows; k++) { lo[k] = 0; hi[k] = nb - 1; }
#pragma unroll 1
  for (int step = 0; step < 8; step++) {   // bin_of_staged<kMsRows, 8>, spelled out
#pragma unroll
    for (int k = 0; k < kMsRows; k++) {
      const int mid = (lo[k] + hi[k] + 1) >> 1;
      const bool le = s_start[mid] <= (unsigned)(k * kThreads + t);
      lo[k] = le ? mid : lo[k];
      hi[k] = le ? hi[k] : mid - 1;
    }
  }
  int id[kMsRows];
  unsigned short j[kMsRows];
#pragma unroll
  for (int k = 0; k < kMsRows; k++) {
    const int lp = k * kThreads + t;
    id[k] = 0; j[k] = 0;
    if (lp < tile_n) {
      const int64_t e = (int64_t)s_goff[lo[k]] + lp;
      id[k] = __builtin_nontemporal_load(&rec_id[e]);
      j[k] = __builtin_nontemporal_load(&rec_j[e]);
    }
  }
#pragma unroll
  for (int k = 0; k < kMsRows; k++)
    if (k * kThreads + t < tile_n) s_out[j[k]] = id[k];
  __syncthreads();
  store_staged<kMsRows>(s_out, tile_n, rec_id1, r.lo);
}

// (option encode_unperm2_group: 4 = default.  Built last in round 3: 2^24 keys 2.64 → 2.60 ms)  Block b serves the b-th GROUP in the
// class-major parent order of the tile numbering; needs nparents ≤ 64 (the two-cut path always has 64): one wave scans the tiles and
// the groups per parent side by side.
template <int G>
__global__ __launch_bounds__(kThreads) void e2_unpermute_group_kernel(const int* __restrict__ rec_id, const unsigned short* __restrict__ rec_j,
                                                                       const unsigned* __restrict__ cnt, const unsigned* __restrict__ toffs, int64_t n,
                                                                       const unsigned* __restrict__ pstart, int nparents, int nb, int* __restrict__ rec_id1) {
  static_assert(G >= 2 && G <= 4, "cumulative counts of up to three earlier tiles");
  __shared__ unsigned s_tiles[64], s_tstart[64], s_gstart[64];
  __shared__ unsigned s_cnt[kThreads], s_start[kThreads], s_goff[kThreads], s_wsum[kThreads / 64];
  __shared__ unsigned s_cum[G - 1][128];
  __shared__ int s_out[G * kMsTile];
  __shared__ int s_pick;
  const int t = threadIdx.x;
  if (t < 64) {
    const unsigned tiles = t < nparents ? ms_tiles_of(pstart, nullptr, t, nparents) : 0u;
    const unsigned groups = (tiles + G - 1) / G;
    unsigned it = tiles, ig = groups;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned a = __shfl_up(it, o, 64), b = __shfl_up(ig, o, 64);
      if (t >= o) { it += a; ig += b; }
    }
    s_tiles[t] = tiles; s_tstart[t] = it - tiles; s_gstart[t] = ig - groups;
  }
  if (t == 0) s_pick = -1;
  __syncthreads();
  if (t < nparents) {
    const unsigned groups = (s_tiles[t] + G - 1) / G;
    if (groups && s_gstart[t] <= blockIdx.x && blockIdx.x < s_gstart[t] + groups) s_pick = t;
  }
  __syncthreads();
  const int j = s_pick;
  if (j < 0) return;
  const int p = ms_parent_of(j, nparents);
  const unsigned g = blockIdx.x - s_gstart[j];
  const int64_t vt0 = (int64_t)s_tstart[j] + (int64_t)g * G;
  const int gt = (int)(s_tiles[j] - g * G < (unsigned)G ? s_tiles[j] - g * G : (unsigned)G);   // tiles in this group
  const int64_t lo = (int64_t)pstart[p] + (int64_t)g * G * kMsTile;
  const int64_t pend = (int64_t)pstart[p + 1], hi = lo + (int64_t)gt * kMsTile < pend ? lo + (int64_t)gt * kMsTile : pend;
  e2_unpermute_body<G>(rec_id, rec_j, cnt, toffs, nb, vt0, gt, lo, (int)(hi - lo), s_cnt, s_start, s_goff, s_wsum, s_cum, s_out, rec_id1);
}

}  // namespace

// Called by encode_core (ah_hash.hip) for 8-byte keys.  lp = log2 of the number of partitions (8 … 10).  *used = 1: out_* hold the
// result; 0: not applicable or the attempt was void (a partition outgrew its table, or one partition holds several times its
// share of the rows) — nothing the caller owns was touched except out_ids / out_dict / out_first_rows, which it rewrites.
// ---- the first look: distinct keys among the first rows, exactly, in one launch ---------------------------------------------------
// What decides "global table or partitions, and how many" is the number of distinct keys among the first 2^16 rows (the urn model
// turns it into the column's expected cardinality, ah_hash.hip).  The global-table path gets that number as a by-product of its
// staged inserts — behind a table fill of tens of MiB, two insert launches and a polled read, ≈ 90 µs that a call which then goes to
// the partitions has spent for nothing (2^20 keys in 2^26 rows: 1.198 ms with the look, 1.105 with the partition count forced,
// profiles/r05_bench_encode_part.json).  This kernel counts the same thing without a table in HBM: kLookWgs workgroups each read all
// `rows` keys (512 KiB out of L2), keep the 1 / kLookWgs of them whose hash names the workgroup, and count those exactly in an LDS set;
// the last workgroup to finish posts the total to the host's mailbox.  The count must be exact: at 2^24 keys the 2^16 rows hold
// ≈ 128 repeats, and a linear-counting bitmap that fits LDS is off by ± 43.
namespace {
constexpr int kLookWgs = 64, kLookSlots = 4096;   // ≤ 2^16 rows: 1024 ± 32 keys per workgroup; keys that find no room count as new ("too many to tell")
__global__ __launch_bounds__(kThreads) void enc_look_kernel(const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ valid, int64_t off, int64_t rows,
                                                            unsigned long long* __restrict__ acc, unsigned* __restrict__ done, unsigned long long* mb,
                                                            unsigned long long seq) {
  __shared__ unsigned long long l_key[kLookSlots];
  __shared__ unsigned s_new, s_last, s_ones;
  const int t = threadIdx.x;
  for (int j = t; j < kLookSlots; j += kThreads) l_key[j] = kEmpty;
  if (t == 0) { s_new = 0; s_ones = 0; }
  __syncthreads();
  unsigned mine = 0;
  // Only 1 / 64 of the rows are this workgroup's: a lane that probed as soon as it met one held its wave for a whole probe sequence
  // — in two of three steps SOME lane has one — and the pass was forty serial LDS round trips per wave (32 µs).  The wave's rows of
  // interest are queued (ballot + prefix count, LDS) and probed together once the queue holds a wave's worth.
  __shared__ unsigned long long s_queue[kThreads / 64][128];
  const int lane = t & 63, wave = t >> 6;
  unsigned long long* q = s_queue[wave];
  int queued = 0;   // (wave-uniform)
  auto insert = [&](unsigned long long key) {
    if (key == kEmpty) { if (atomicExch(&s_ones, 1u) == 0u) mine++; return; }   // the all-ones key is the set's empty marker: counted on the side
    const unsigned m = ((unsigned)key ^ ((unsigned)(key >> 32) * 0x9E3779B1u)) * 0x85EBCA6Bu;
    unsigned j = (m >> 10) & (unsigned)(kLookSlots - 1);
    bool placed = false;
    for (int probes = 0; probes < kLookSlots && !placed; probes++) {
      unsigned long long cur = l_key[j];
      if (cur == kEmpty) cur = atomicCAS(&l_key[j], kEmpty, key);
      if (cur == kEmpty) { mine++; placed = true; }
      else if (cur == key) placed = true;
      j = (j + 1) & (unsigned)(kLookSlots - 1);
    }
    if (!placed) mine++;
  };
  auto drain = [&](int from) {   // the queue's entries from `from` on, one per lane
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (from + lane < queued) insert(q[from + lane]);
    __builtin_amdgcn_wave_barrier();
  };
  constexpr int U = 16;   // loads in flight per lane: the pass is four round trips to L2 long
  for (int64_t b = 0; b < rows; b += (int64_t)kThreads * U) {
    unsigned long long k[U];
#pragma unroll
    for (int u = 0; u < U; u++) { const int64_t i = b + u * kThreads + t; k[u] = i < rows ? keys[i] : 0ull; }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = b + u * kThreads + t;
      // a 32-bit hash (two quarter-rate multiplies): every workgroup hashes ALL the rows
      const unsigned m = ((unsigned)k[u] ^ ((unsigned)(k[u] >> 32) * 0x9E3779B1u)) * 0x85EBCA6Bu;
      const bool in = i < rows && ah_bit(valid, off + i) && (m >> 26) == blockIdx.x;   // kLookWgs = 64: the top six bits
      const unsigned long long mask = __ballot(in);
      if (in) q[queued + __popcll(mask & ((1ull << lane) - 1ull))] = k[u];
      queued += __popcll(mask);
      if (queued >= 64) {   // (uniform) at most 127 queued: the first 64 go now
        drain(0);
        const unsigned long long rest = lane + 64 < queued ? q[lane + 64] : 0ull;
        __builtin_amdgcn_wave_barrier();
        if (lane + 64 < queued) q[lane] = rest;
        queued -= 64;
      }
    }
  }
  drain(0);
  if (mine) atomicAdd(&s_new, mine);
  __syncthreads();
  if (t == 0) {
    atomicAdd(acc, (unsigned long long)s_new);
    __threadfence();
    s_last = atomicAdd(done, 1u) == gridDim.x - 1u ? 1u : 0u;
    if (s_last) {
      __threadfence();
      const unsigned long long w = __hip_atomic_exchange(acc, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // both words are left zero for the next call
      __hip_atomic_store(done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ah_mailbox_post(mb, seq, &w, 1);
    }
  }
}

}  // namespace
// distinct valid keys among the first `rows` (≤ 2^16) rows → *distinct.  One launch and a polled wait.
int ah_encode_first_look(ah_ctx* c, const uint64_t* keys, const uint8_t* valid, int64_t off, int64_t rows, uint64_t* distinct) {
  unsigned long long* acc = (unsigned long long*)&c->dscalars[kDsEncLook];   // the count and (kDsEncLookDone) the workgroups that have finished: zero on entry, zeroed again by the last workgroup
  unsigned long long *mb, seq, w;
  int rc = ah_mailbox_begin(c, &mb, &seq);
  if (rc != AH_OK) return rc;
  enc_look_kernel<<<kLookWgs, kThreads, 0, c->stream>>>((const unsigned long long*)keys, valid, off, rows, acc, (unsigned*)&c->dscalars[kDsEncLookDone], mb, seq);
  AH_LAUNCH_CHECK(c);
  if ((rc = ah_mailbox_wait(c, seq, 1, &w)) != AH_OK) return rc;
  *distinct = (uint64_t)w;
  return AH_OK;
}

// ---- the host drivers ---------------------------------------------------------------------------------------------------------------
namespace {
// One unique / dictionary_encode call as the two drivers see it (the exported signatures' common tuple)
struct EncCall {
  ah_ctx* c;
  const unsigned long long* keys; const uint8_t* valid; int64_t off, n;
  int encode_nulls, lp, slots;
  int32_t* out_ids; uint64_t* out_dict; int64_t* out_first_rows;
  int64_t* out_ndict; int32_t* out_null_id;   // host
  // the call's words of dscalars
  unsigned* flags() const { return (unsigned*)&c->dscalars[kDsEncFlags]; }   // kPartOverflow: a partition held more keys than its table admits
  unsigned long long* total() const { return (unsigned long long*)&c->dscalars[kDsEncTotal]; }
  int* null_id() const { return (int*)&c->dscalars[kDsEncNullId]; }
};
// `slots` (kESlots or kESlots2: the drivers have checked) as a compile-time constant: f(std::integral_constant<int, slots>{})
template <class F>
void with_slots(int slots, F&& f) {
  if (slots == kESlots2) f(std::integral_constant<int, kESlots2>{});
  else f(std::integral_constant<int, kESlots>{});
}

// What both drivers do behind their cut — the partitions' tables, the first-occurrence bitmap and its ranks, the dictionary, the
// records' ids — and the temporaries of that part.
struct EncTables {
  int64_t nslots, nwords, nrt;
  unsigned long long *tab_key, *firsts;
  unsigned *tab_first, *wordprefix; unsigned short* rec_slot; int* tilecnt; int64_t* tileoff;
  uint8_t* fbytes;   // first occurrences marked by plain byte stores, packed into `firsts` by one pass; null: atomicOr on the bitmap's words
  EncTables(const EncCall& e, int64_t P) : nslots(P * (e.slots + 8)), nwords(ah_ceil_div(e.n, 64)), nrt(rank_tiles(nwords)) {}
  void carve(TempCarver& tc, int64_t n, bool byte_map) {
    tc.take(rec_slot, n); tc.take(tab_key, nslots); tc.take(tab_first, nslots); tc.take(firsts, nwords);
    fbytes = byte_map ? tc.take((size_t)nwords * 64) : nullptr;
    tc.take(wordprefix, nwords); tc.take(tilecnt, nrt); tc.take(tileoff, nrt);
  }
  // the call's scalars and the map the first occurrences are marked in: one launch where three memsets were (≈ 4 µs of gap each)
  int fill(const EncCall& e) const {
    GbFill f;
    f.njobs = 2;
    f.p[0] = (uint4*)e.flags(); f.n16[0] = 1; f.v[0] = 0u;                       // flags, total
    f.ones = (unsigned long long*)e.null_id();                                   // null id: none
    if (fbytes) { f.p[1] = (uint4*)fbytes; f.n16[1] = (size_t)nwords * 4; }   // the byte map (the bitmap is then written whole)
    else { f.p[1] = (uint4*)firsts; f.n16[1] = ah_pad((size_t)nwords * 8) / 16; }
    f.v[1] = 0u;
    gb_fill_kernel<<<(unsigned)(e.c->num_cu * 2), 256, 0, e.c->stream>>>(f);
    AH_LAUNCH_CHECK(e.c);
    return AH_OK;
  }
  // tables (one workgroup per final partition), ranks, the dictionary and — when ids are wanted — every record's id in rec_id
  int run(const EncCall& e, int64_t P, const unsigned long long* pkeys, const unsigned* prows, const unsigned* binstart, bool batch, bool compact, int* rec_id) const {
    ah_ctx* c = e.c;
    unsigned long long* tab_key_out = compact ? nullptr : tab_key;
    with_slots(e.slots, [&](auto s) { with_bool(batch, [&](auto b) {
      enc_table_kernel<s.value, b.value><<<(unsigned)P, kThreads, 0, c->stream>>>(pkeys, prows, binstart, e.encode_nulls, tab_key_out, tab_first, e.out_ids ? rec_slot : nullptr, firsts, e.flags(), fbytes);
    }); });
    AH_LAUNCH_CHECK(c);
    if (fbytes) {
      enc_bytes_to_bits_kernel<<<(unsigned)ah_ceil_div(nwords, kBlock), kBlock, 0, c->stream>>>(fbytes, nwords, firsts);
      AH_LAUNCH_CHECK(c);
    }
    word_prefix_kernel<<<(unsigned)ah_ceil_div(nwords, kBlock), kBlock, 0, c->stream>>>(firsts, nwords, wordprefix, tilecnt);
    AH_LAUNCH_CHECK(c);
    scan_kernel<<<1, 1024, 0, c->stream>>>(tilecnt, nrt, tileoff, e.total());
    AH_LAUNCH_CHECK(c);
    const int rc = enc_emit(c, compact, e.out_ids != nullptr, tab_key, tab_first, nslots, firsts, wordprefix, tileoff, (const uint64_t*)e.keys, e.n, e.out_dict, e.out_first_rows, e.null_id(), e.slots);
    if (rc != AH_OK || !e.out_ids) return rc;
    const int rsplit = P >= c->opt_encode_resolve_wgs ? 1 : (int)(c->opt_encode_resolve_wgs / P);   // ≥ 1024 workgroups: one per partition leaves a CU 16 waves
    with_slots(e.slots, [&](auto s) { enc_resolve_kernel<s.value><<<(unsigned)(P * rsplit), kThreads, 0, c->stream>>>(rec_slot, tab_first, binstart, rec_id, rsplit); });
    AH_LAUNCH_CHECK(c);
    return AH_OK;
  }
};
// {flags, total, null id} home → *used and the two host outputs.  A set flag: the global-table path redoes the call.
int enc_finish(const EncCall& e, int* used) {
  PartOutcome outcome;
  const int rc = part_finish(e.c, kDsEncFlags, false, e.out_ndict, e.out_null_id, &outcome);
  if (rc == AH_OK) *used = outcome == PartOutcome::Done;
  return rc;
}
}  // namespace

int ah_encode_partitioned_try(ah_ctx* c, const uint64_t* keys, const uint8_t* valid, int64_t off, int64_t n, int encode_nulls, int lp, int slots,
                              int32_t* out_ids, uint64_t* out_dict, int64_t* out_first_rows, int64_t* out_ndict, int32_t* out_null_id, int* used) {
  *used = 0;
  if (n < 1 || n >= kMaxRows || lp < 3 || lp > 10 || (slots != kESlots && slots != kESlots2)) return AH_OK;
  const EncCall e{c, (const unsigned long long*)keys, valid, off, n, encode_nulls, lp, slots, out_ids, out_dict, out_first_rows, out_ndict, out_null_id};
  const int P = 1 << lp;
  const int64_t ntiles = ah_ceil_div(n, kGbTile), ngrp = ah_ceil_div(ntiles, kGroupTiles);
  // (the byte map from 1024 partitions on — ≈ 4·10^6 keys: below, the map's fill and packing cost what the atomics cost)
  const bool byte_map = c->opt_encode_byte_map == 2 || (c->opt_encode_byte_map == 1 && lp >= 10);
  EncTables t(e, P);
  unsigned *cnt_tm, *toffs, *gsum, *binstart, *prows;
  uint8_t* kbase = nullptr;   // the records' keys from the scatter until the table pass has given every record its slot, then their ids
  bool fits;
  int rc = part_reserve(c, false, [&](TempCarver& tc) {
    tc.take(cnt_tm, (size_t)P * ntiles); tc.take(toffs, (size_t)P * ntiles); tc.take(gsum, ngrp * P); tc.take(binstart, P + 1);
    kbase = tc.take((size_t)n * 8);
    tc.take(prows, n);
    t.carve(tc, n, byte_map);
  }, &fits);
  if (rc != AH_OK) return rc;
  unsigned long long* pkeys = (unsigned long long*)kbase;
  int* rec_id = (int*)kbase;
  if ((rc = t.fill(e)) != AH_OK) return rc;
  // ---- 1, 2: cut
  const unsigned tgrid = (unsigned)(((ntiles + 7) / 8) * 8);
  gb_hist_kernel<<<tgrid, kGbHistThreads, 0, c->stream>>>(e.keys, valid, off, n, lp, P, ntiles, cnt_tm);
  AH_LAUNCH_CHECK(c);
  // one workgroup per partition is only as fast as the largest partition: the sizes are looked at before the tables are built — through
  // the mailbox, posted by the prefix kernel itself and read while the offsets and the scatter are already running (a copy of
  // binstart + a stream synchronisation left the device idle for ≈ 15 µs on every call; a lopsided column now costs a scatter
  // that nobody reads, and such columns rarely get here: the first look sends them to the global table)
  unsigned long long *mb, seq, largest = 0;
  if ((rc = ah_mailbox_begin(c, &mb, &seq)) != AH_OK) return rc;
  if ((rc = launch_tile_offsets(c, cnt_tm, P, ntiles, n, gsum, toffs, binstart, mb, seq)) != AH_OK) return rc;
  gb_scatter_kernel<false><<<tgrid, kThreads, 0, c->stream>>>(e.keys, valid, off, nullptr, nullptr, 0, n, lp, P, ntiles, toffs, pkeys, nullptr, prows, nullptr);
  AH_LAUNCH_CHECK(c);
  if ((rc = ah_mailbox_wait(c, seq, 1, &largest)) != AH_OK) return rc;
  if ((int64_t)largest * P > 3 * n && largest > (1u << 16)) return AH_OK;
  // ---- 3, 4, 5: tables, ranks, ids per record
  // (measured at 2^26 rows: from 2^22 keys on — 1024 partitions — the compaction wins; below, the slots' few scattered stores are cheaper than its pass)
  const bool compact = c->opt_encode_dict_compact >= 2 || (c->opt_encode_dict_compact == 1 && lp >= 10);
  if ((rc = t.run(e, P, pkeys, prows, binstart, c->opt_encode_table_batch != 0, compact, rec_id)) != AH_OK) return rc;
  if (out_ids) {   // ---- 6: ids per row
    launch_enc_unpermute(c, rec_id, prows, cnt_tm, toffs, P, ntiles, n, out_ids);
    AH_LAUNCH_CHECK(c);
  }
  return enc_finish(e, used);
}

// Two cuts: 64 parents × 2^(lp − 6) partitions (lp = 11 … 13), for ≈ 4.5 … 36 M expected keys.  Same contract as above.
int ah_encode_partitioned2_try(ah_ctx* c, const uint64_t* keys, const uint8_t* valid, int64_t off, int64_t n, int encode_nulls, int lp, int slots,
                               int32_t* out_ids, uint64_t* out_dict, int64_t* out_first_rows, int64_t* out_ndict, int32_t* out_null_id, int* used) {
  *used = 0;
  if (n < ((int64_t)1 << 20) || n >= kMaxRows || lp < 7 || lp > 13 || (slots != kESlots && slots != kESlots2)) return AH_OK;
  const EncCall e{c, (const unsigned long long*)keys, valid, off, n, encode_nulls, lp, slots, out_ids, out_dict, out_first_rows, out_ndict, out_null_id};
  constexpr int lb1 = 6, nb1 = 1 << lb1;
  const int lb2 = lp - lb1, nb2 = 1 << lb2;
  const int64_t P = (int64_t)1 << lp;
  const int64_t ntiles = ah_ceil_div(n, kGbTile), ngrp = ah_ceil_div(ntiles, kGroupTiles), nvt = ((ntiles + nb1 + 7) / 8) * 8;
  EncTables t(e, P);
  unsigned *cnt1, *toffs1, *gsum, *pstart, *cnt2, *toffs2, *bstart, *prows1, *prows2;
  unsigned short* pj2;
  TileRange* tile_table;
  // each level's keys, then its records' ids: level 1's are dead after the level-2 scatter, level 2's once every record knows its slot
  uint8_t *kbase1 = nullptr, *kbase2 = nullptr;
  bool fits;
  int rc = part_reserve(c, false, [&](TempCarver& tc) {
    tc.take(cnt1, ntiles * nb1); tc.take(toffs1, ntiles * nb1); tc.take(gsum, ngrp * nb1); tc.take(pstart, nb1 + 1);
    tc.take(cnt2, nvt * nb2); tc.take(toffs2, nvt * nb2); tc.take(bstart, P + 1);
    kbase1 = tc.take((size_t)n * 8); kbase2 = tc.take((size_t)n * 8);
    tc.take(prows1, n); tc.take(prows2, n); tc.take(pj2, n);
    t.carve(tc, n, c->opt_encode_byte_map != 0);
    tc.take(tile_table, nvt);
  }, &fits);
  if (rc != AH_OK) return rc;
  unsigned long long *pkeys1 = (unsigned long long*)kbase1, *pkeys2 = (unsigned long long*)kbase2;
  int *rec_id1 = (int*)kbase1, *rec_id2 = (int*)kbase2;
  if ((rc = t.fill(e)) != AH_OK) return rc;
  // ---- level 1: 64 parents by the top 6 bits of the key hash
  const unsigned tgrid = (unsigned)(((ntiles + 7) / 8) * 8);
  gb_hist_kernel<<<tgrid, kGbHistThreads, 0, c->stream>>>(e.keys, valid, off, n, lb1, nb1, ntiles, cnt1);
  AH_LAUNCH_CHECK(c);
  if ((rc = launch_tile_offsets(c, cnt1, nb1, ntiles, n, gsum, toffs1, pstart)) != AH_OK) return rc;
  gb_scatter_kernel<false><<<tgrid, kThreads, 0, c->stream>>>(e.keys, valid, off, nullptr, nullptr, 0, n, lb1, nb1, ntiles, toffs1, pkeys1, nullptr, prows1, nullptr);
  AH_LAUNCH_CHECK(c);
  // ---- level 2: every parent into 2^lb2 partitions
  ms_tile_table_kernel<<<(unsigned)ah_ceil_div(nvt, kThreads), kThreads, 0, c->stream>>>(pstart, nullptr, nb1, (unsigned)nvt, tile_table);
  AH_LAUNCH_CHECK(c);
  tile_hist_kernel<E2Digit><<<(unsigned)nvt, kThreads, 0, c->stream>>>(E2Digit{pkeys1, prows1, lp, (unsigned)(nb2 - 1)}, n, pstart, nb1, nb2, cnt2, tile_table);
  AH_LAUNCH_CHECK(c);
  // (the partitions' balance: posted by the offsets kernel, read while the scatter runs — see ah_encode_partitioned_try)
  unsigned long long *mb, seq, largest = 0;
  if ((rc = ah_mailbox_begin(c, &mb, &seq)) != AH_OK) return rc;
  ms_offs2_kernel<<<(unsigned)nb1, kThreads, 0, c->stream>>>(cnt2, pstart, nb1, nb2, toffs2, bstart, n, (unsigned*)&c->dscalars[kDsEncLargest], (unsigned*)&c->dscalars[kDsEncLargestDone], mb, seq);
  AH_LAUNCH_CHECK(c);
  e2_scatter_kernel<<<(unsigned)nvt, kThreads, 0, c->stream>>>(pkeys1, prows1, n, pstart, nb1, lp, (unsigned)(nb2 - 1), nb2, toffs2, pkeys2, prows2, pj2);
  AH_LAUNCH_CHECK(c);
  if ((rc = ah_mailbox_wait(c, seq, 1, &largest)) != AH_OK) return rc;
  if ((int64_t)largest * P > 3 * n && largest > (1u << 16)) return AH_OK;   // a key that owns a large share of the rows: the other path
  // ---- tables, ranks, ids per record: as in the one-level path (small partitions: the batched probe's registers cost more than its waits)
  if ((rc = t.run(e, P, pkeys2, prows2, bstart, false, c->opt_encode_dict_compact >= 1, rec_id2)) != AH_OK) return rc;
  if (out_ids) {   // ---- ids home: virtual tile by virtual tile into level-1 order, then tile by tile into row order
    if (c->opt_encode_unperm2_group >= 2 && nb1 <= 64 && nb2 <= 128)
      e2_unpermute_group_kernel<4><<<(unsigned)(ah_ceil_div(ntiles + nb1, 4) + nb1), kThreads, 0, c->stream>>>(rec_id2, pj2, cnt2, toffs2, n, pstart, nb1, nb2, rec_id1);
    else
      e2_unpermute_kernel<<<(unsigned)nvt, kThreads, 0, c->stream>>>(rec_id2, pj2, cnt2, toffs2, n, pstart, nb1, nb2, rec_id1);
    AH_LAUNCH_CHECK(c);
    launch_enc_unpermute(c, rec_id1, prows1, cnt1, toffs1, nb1, ntiles, n, out_ids);
    AH_LAUNCH_CHECK(c);
  }
  return enc_finish(e, used);
}
