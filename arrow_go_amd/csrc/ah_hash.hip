// ah_hash.hip — unique / dictionary_encode over 8-byte and byte-string keys; the dense group ids of the id-based group-by (ah_hash_agg.hip).
//
// Replaces: doAppendNumeric[uint64] (kernels/vector_hash.go:359-385) driving
//   hashing.Table[uint64].InsertOrGet / GetOrInsertNull
//   (internal/hashing/xxh3_memo_table_types.go:231-238,283-294; open-addressing table
//   :45-187; hashInt internal/hashing/hash_funcs.go:60-67), the
//   dictionaryEncodeAction (vector_hash.go:145-241) and uniqueFinalize (:721-741),
//   behind compute's "unique" / "dictionary_encode" (compute/vector_hash.go:61,79).
//   Int64 and Float64 columns both hash raw 64-bit patterns (vector_hash.go:604-607).
//
// The reference is strictly sequential: memo index = order of first insertion.  The
// same ids are produced in parallel as follows:
//   1. insert_kernel  — every row CASes its key into an open-addressing table keyed
//      by the reference's hashInt (linear probing; 16-byte slots {key, first_row,
//      id}) and atomicMin's its row number into the slot: first_row = first
//      occurrence.  The all-ones key (the table's EMPTY marker) and the null key live
//      in two dedicated slots past the end.  Plain loads short-circuit both atomics
//      once a slot is settled, so low-cardinality columns do not serialise on L2.
//   2. mark_kernel    — each used slot sets bit first_row in an n-bit "first
//      occurrence" bitmap.
//   3. rank kernels   — prefix popcount of that bitmap (per-64-row word prefixes inside
//      2048-row tiles + one scan of tile totals): the number of first occurrences
//      before row r IS the sequential memo index of the key first seen at row r.
//   4. assign_kernel  — each used slot computes its id from (3) and writes its key to
//      dict[id].
//   5. emit_kernel    — out_ids[i] = id of row i's slot (remembered in step 1).
// If more than cap/2 distinct keys show up the attempt is abandoned and repeated
// with a 16× larger table (the reference grows ×4 at the same load factor,
// xxh3_memo_table_types.go:109,169-179); results never depend on the capacity.
//
// HBM: 8 B/row of keys + random 16-byte slot traffic (atomics-bound at high
// cardinality, cache-resident at low cardinality).
#include "ah_common.h"
#include "ah_hashing.h"
#include "ah_bytes.h"

namespace {


struct Slot {
  unsigned long long key;
  unsigned first_row;
  unsigned id;
};


// ---- what a "key" is -------------------------------------------------------------------------------
// The table machinery below (insert → rank → emit) only needs, per row: a 64-bit word to CAS into an empty
// slot, a hash to start probing at, and "does this occupied slot hold my key".
struct U64Keys {  // Table[uint64] (xxh3_memo_table_types.go): the word is the key itself
  const unsigned long long* keys;
  static constexpr bool kLdsTable = true;
  // false → the all-ones key, which doubles as the EMPTY marker and lives in its own slot
  __device__ __forceinline__ bool load(int64_t i, unsigned long long* word, uint64_t* h) const {
    const unsigned long long k = keys[i];
    *word = k;
    *h = hash_int(k);
    return k != kEmpty;
  }
  __device__ __forceinline__ bool same(unsigned long long cur, unsigned long long word, int64_t) const { return cur == word; }
};

// BinaryMemoTable (internal/hashing/xxh3_memo_table.go): the slot word is {hash bits 63..32 | a row that
// holds the value}; a slot is "mine" when the tags agree and the bytes of that row equal mine.  Both
// halves arrive in one CAS, so a reader never sees a tag without its row.  Rows are read through ah_bytes.h's
// ByteRows: OW = 4 / 8 for String / Binary / LargeString / LargeBinary, OW = 0 for FixedSizeBinary / Decimal128 /
// Decimal256 keys (kernels/vector_hash.go:608-609, 698: the same BinaryMemoTable, every value `w` bytes).
template <int OW>
struct ByteKeys {
  ByteRows rows;  // of row 0 of the call
  static constexpr bool kLdsTable = false;
  __device__ __forceinline__ bool load(int64_t i, unsigned long long* word, uint64_t* h) const {
    const uint8_t* p;
    int64_t len;
    row_at<OW>(rows, i, &p, &len);
    *h = hash_bytes(p, len);
    *word = (*h & 0xFFFFFFFF00000000ull) | (unsigned long long)(unsigned)i;  // never all-ones: i < 2^32 − 1
    return true;
  }
  __device__ __forceinline__ bool same(unsigned long long cur, unsigned long long word, int64_t i) const {
    if ((cur ^ word) >> 32) return false;
    const int64_t r = (int64_t)(unsigned)cur;
    if (r == i) return true;
    const uint8_t *p, *q;
    int64_t len, qlen;
    row_at<OW>(rows, i, &p, &len);
    row_at<OW>(rows, r, &q, &qlen);
    return len == qlen && equal_bytes(p, q, len);
  }
};

// A key that is a TUPLE of columns (ah_group_ids, ah_group_keys.hip; no reference analogue — DESIGN.md §3.2).  The slot word is
// {hash bits 63..32 | a row that holds the tuple}, as for ByteKeys; no row is materialised: load() hashes the row's columns where
// they lie and same() compares them column by column — null flags first (two nulls are equal, the payload under a null is never
// read), lengths before bytes.  NC is a compile-time bound (2, 4 or 8; unused entries are kColNone), so col[] is indexed
// statically and stays in scalar registers.
enum : int { kColNone = 0, kColFixed = 1, kColBits = 2, kColVar4 = 4, kColVar8 = 8 };
struct KeyCol {
  const void* offsets;   // kColVar4 / 8: the offsets entry of row 0 of the call
  const uint8_t* data;   // kColVar*: the data buffer; kColFixed: the slot of row 0 of the call; kColBits: the bitmap (bit off + i)
  const uint8_t* valid;  // nullable; bit off + i
  int64_t off;
  int kind, w;           // w: bytes per slot of a kColFixed column
};
constexpr uint64_t kNullColHash = 0xA0761D6478BD642Full, kTrueColHash = 0xE7037ED1A0B428DBull, kFalseColHash = 0x8EBC6AF09C88C6E3ull;

__device__ __forceinline__ void col_row(const KeyCol& k, int64_t i, const uint8_t** p, int64_t* len) {
  if (k.kind == kColVar4) row_at<4>(ByteRows{k.offsets, k.data, 0}, i, p, len);
  else if (k.kind == kColVar8) row_at<8>(ByteRows{k.offsets, k.data, 0}, i, p, len);
  else row_at<0>(ByteRows{nullptr, k.data, k.w}, i, p, len);
}

template <int NC>
struct TupleKeys {
  KeyCol col[NC];
  static constexpr bool kLdsTable = false;
  __device__ __forceinline__ bool load(int64_t i, unsigned long long* word, uint64_t* h) const {
    uint64_t acc = 0x9E3779B97F4A7C15ull;
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const KeyCol& k = col[c];
      if (k.kind == kColNone) continue;
      uint64_t hc;
      if (!ah_bit(k.valid, k.off + i)) {
        hc = kNullColHash;
      } else if (k.kind == kColBits) {
        hc = ah_bit(k.data, k.off + i) ? kTrueColHash : kFalseColHash;
      } else {
        const uint8_t* p;
        int64_t len;
        col_row(k, i, &p, &len);
        hc = hash_bytes(p, len);
      }
      acc = (acc ^ hc) * 0xFF51AFD7ED558CCDull;   // order matters: ("ab", "c") and ("c", "ab") start their probes apart
      acc ^= acc >> 32;
    }
    *h = acc;
    *word = (acc & 0xFFFFFFFF00000000ull) | (unsigned long long)(unsigned)i;  // never all-ones: i < 2^32 − 1
    return true;
  }
  __device__ __forceinline__ bool same(unsigned long long cur, unsigned long long word, int64_t i) const {
    if ((cur ^ word) >> 32) return false;
    const int64_t r = (int64_t)(unsigned)cur;
    if (r == i) return true;
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const KeyCol& k = col[c];
      if (k.kind == kColNone) continue;
      const int vi = ah_bit(k.valid, k.off + i), vr = ah_bit(k.valid, k.off + r);
      if (vi != vr) return false;
      if (!vi) continue;
      if (k.kind == kColBits) {
        if (ah_bit(k.data, k.off + i) != ah_bit(k.data, k.off + r)) return false;
      } else {
        const uint8_t *p, *q;
        int64_t len, qlen;
        col_row(k, i, &p, &len);
        col_row(k, r, &q, &qlen);
        if (len != qlen || !equal_bytes(p, q, len)) return false;
      }
    }
    return true;
  }
};

// dictionary of fixed-width keys: entry id = the value at its first row (the null entry: zeros, like a fresh builder slot)
__global__ __launch_bounds__(kBlock) void fixed_dict_kernel(const uint8_t* __restrict__ data, int w, const long long* __restrict__ first_rows, int64_t ndict,
                                                             int null_id, uint8_t* __restrict__ dict) {
  const int64_t total = ndict * w;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < total; b += stride) {
    const int64_t id = b / w;
    dict[b] = id == null_id ? (uint8_t)0 : data[first_rows[id] * w + (b - id * w)];
  }
}

// status words in dscalars: [4] distinct count, [5] overflow flag, [6] total ids
// Inserts rows [lo, hi).  Probe chains longer than kProbeLimit mean the table is far beyond
// the load it was sized for (at load ≤ ½ the chance of a 256-long linear-probing cluster is
// ≈ 0.82^256 ≈ 1e-22 per insert) → flag overflow; the host retries with a larger table.
constexpr int kProbeLimit = 256;

constexpr int kInsertRows = 4;  // independent rows per lane per step: their first probes are in flight together

struct SlotView {  // one 16-byte load: the fields of a slot as they were at (about) the same time
  unsigned long long key;
  unsigned first_row;
  unsigned id;
};
__device__ __forceinline__ SlotView load_slot(const Slot* p) {
  const uint4 v = *reinterpret_cast<const uint4*>(p);
  return SlotView{((unsigned long long)v.y << 32) | v.x, v.z, v.w};
}

template <typename K>
__global__ __launch_bounds__(kBlock) void insert_kernel(const K keys, const uint8_t* __restrict__ valid,
                                                         int64_t off, int64_t lo, int64_t hi, int encode_nulls, Slot* __restrict__ table,
                                                         uint64_t cap, unsigned* __restrict__ row_slot, unsigned flag, unsigned direct_below,
                                                         unsigned long long* __restrict__ distinct, unsigned* __restrict__ overflow,
                                                         unsigned long long* __restrict__ misses) {
  // direct_below > 0: the slots whose first_row lies below it have been ranked already (their id is final,
  // see encode_core) — such a row gets its id right here, every other row a slot number with `flag` set.
  const uint64_t mask = cap - 1;
  const int64_t stride = (int64_t)gridDim.x * kBlock * kInsertRows;
  unsigned nmiss = 0;
  unsigned fresh = 0;  // keys this lane inserted (published once, at the end: same-address atomics cost ~12 ns each)
  for (int64_t base = lo + (int64_t)blockIdx.x * kBlock * kInsertRows + threadIdx.x; base < hi; base += stride) {
    // kind: 0 = nothing to do, 1 = probe the table, 2 = dedicated slot (all-ones key / null), 3 = masked null
    int kind[kInsertRows];
    unsigned long long k[kInsertRows];  // the word this row would CAS into an empty slot
    uint64_t idx[kInsertRows];
    SlotView sv[kInsertRows];
#pragma unroll
    for (int u = 0; u < kInsertRows; u++) {
      const int64_t i = base + (int64_t)u * kBlock;
      kind[u] = 0;
      k[u] = 0;
      idx[u] = 0;
      if (i < hi) {
        if (ah_bit(valid, off + i)) {
          uint64_t h;
          if (!keys.load(i, &k[u], &h)) { kind[u] = 2; idx[u] = cap; }
          else { kind[u] = 1; idx[u] = h & mask; }
        } else if (encode_nulls) { kind[u] = 2; idx[u] = cap + 1; }
        else kind[u] = 3;
      }
    }
#pragma unroll
    for (int u = 0; u < kInsertRows; u++)
      if (kind[u] == 1 || kind[u] == 2) sv[u] = load_slot(&table[idx[u]]);
#pragma unroll
    for (int u = 0; u < kInsertRows; u++) {
      const int64_t i = base + (int64_t)u * kBlock;
      if (kind[u] == 0) continue;
      if (kind[u] == 3) { if (row_slot) row_slot[i] = direct_below ? 0u : kNoRow; continue; }  // masked null → index 0, now or in emit_kernel
      uint64_t s = idx[u];
      unsigned fr = sv[u].first_row;  // may be stale — only ever LARGER than the truth, so the atomicMin below stays correct
      unsigned id = sv[u].id;
      if (kind[u] == 1) {
        unsigned long long cur = sv[u].key;
        int probes = 0;
        for (;;) {
          if (cur == kEmpty) {  // settled slots skip the CAS
            cur = atomicCAS(&table[s].key, kEmpty, k[u]);
            if (cur == kEmpty) { fresh++; break; }
          }
          if (keys.same(cur, k[u], i)) break;
          s = (s + 1) & mask;
          if (++probes > kProbeLimit) { atomicExch(overflow, 1u); return; }
          const SlotView nx = load_slot(&table[s]);
          cur = nx.key;
          fr = nx.first_row;
          id = nx.id;
        }
      }
      if (fr < direct_below) {  // seen in the ranked prefix: nothing to update (i ≥ direct_below > fr)
        if (row_slot) row_slot[i] = id;
        continue;
      }
      if (fr > (unsigned)i) atomicMin(&table[s].first_row, (unsigned)i);
      if (row_slot) row_slot[i] = (unsigned)s | flag;  // flag: bit 31 when emit_kernel must tell slots from final ids
      nmiss++;
    }
  }
  if (fresh) atomicAdd(distinct, (unsigned long long)fresh);
  if (direct_below && nmiss) atomicAdd(misses, (unsigned long long)nmiss);
}

__global__ __launch_bounds__(kBlock) void mark_kernel(const Slot* __restrict__ table, uint64_t nslots,
                                                       unsigned long long* __restrict__ firsts) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < nslots; s += stride) {
    unsigned fr = table[s].first_row;
    if (fr != kNoRow) atomicOr(&firsts[fr >> 6], 1ull << (fr & 63));
  }
}


__global__ __launch_bounds__(kBlock) void assign_kernel(Slot* __restrict__ table, uint64_t cap, const unsigned long long* __restrict__ firsts,
                                                         const unsigned* __restrict__ wordprefix, const int64_t* __restrict__ tileoff,
                                                         unsigned long long* __restrict__ dict, int* __restrict__ null_id,
                                                         long long* __restrict__ first_rows) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const uint64_t nslots = cap + 2;
  for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < nslots; s += stride) {
    unsigned fr = table[s].first_row;
    if (fr == kNoRow) continue;
    unsigned id = rank_of_row(fr, firsts, wordprefix, tileoff);
    table[s].id = id;
    if (first_rows) first_rows[id] = (long long)fr;
    if (s == cap + 1) {
      *null_id = (int)id;
      if (dict) dict[id] = 0;  // GetDictArrayData: the null slot keeps the fresh buffer's zero
    } else if (dict) {
      dict[id] = table[s].key;  // slot `cap` holds the all-ones key: key field is still kEmpty == that key
    }
  }
}

// ids[i] holds what the insert pass left there: a slot number (→ that slot's id), kNoRow (masked null →
// index 0, vector_hash.go:169-172), or — for rows ≥ direct_from, written by insert_small_kernel — either a
// final id (kept) or a slot number flagged with bit 31.
__global__ __launch_bounds__(kBlock) void emit_kernel(const Slot* __restrict__ table, int32_t* __restrict__ ids, int64_t n, int64_t direct_from) {
  constexpr int U = 4;  // gathers in flight per lane
  const int64_t stride = (int64_t)gridDim.x * kBlock * U;
  for (int64_t base = (int64_t)blockIdx.x * kBlock * U + threadIdx.x; base < n; base += stride) {
    unsigned s[U];
    int32_t id[U];
    bool put[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = base + (int64_t)u * kBlock;
      s[u] = i < n ? (unsigned)ids[i] : kNoRow;
      put[u] = i < n;
      if (i >= direct_from && s[u] != kNoRow) {
        if (s[u] & 0x80000000u) s[u] &= 0x7fffffffu; else put[u] = false;
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) id[u] = s[u] == kNoRow ? 0 : (put[u] ? (int32_t)table[s[u]].id : 0);
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = base + (int64_t)u * kBlock;
      if (put[u]) ids[i] = id[u];
    }
  }
}

// ---- what the two cached-lookup kernels below share ------------------------------------------------------------
// Both answer a row from a read-only copy of the ranked prefix's (key → id) pairs and fall back to the insert table for a key the
// prefix did not hold.  Their load scheduling differs (and was measured); the rows the cache does not answer are handled here.
constexpr unsigned kLookup = 0xFFFFFFFEu;   // (no id: ids and flagged slot numbers stay below it)
struct InsertSide {   // what those kernels know of the insert table before their first row
  uint64_t cap;
  int encode_nulls;
  unsigned ones_id, null_id;   // the two dedicated slots (all-ones key, null): final ids if the prefix saw them, else kNoRow
  __device__ __forceinline__ InsertSide(const Slot* t, uint64_t cap_, int encode_nulls_)
      : cap(cap_), encode_nulls(encode_nulls_), ones_id(t[cap_].first_row != kNoRow ? t[cap_].id : kNoRow),
        null_id(t[cap_ + 1].first_row != kNoRow ? t[cap_ + 1].id : kNoRow) {}
};

// The claim loop: walk key k's probe chain in the insert table up to its slot, claiming the first empty one on the way.
// → false: the chain is longer than `limit` (overflow flagged; the host retries with a larger table).
__device__ __forceinline__ bool claim_slot(unsigned long long k, Slot* __restrict__ table, uint64_t mask, int limit, unsigned* __restrict__ overflow,
                                           uint64_t* slot, unsigned* inserted) {
  uint64_t s = hash_int(k) & mask;
  int probes = 0;
  for (;;) {
    unsigned long long cur = table[s].key;
    if (cur != k && cur == kEmpty) {
      cur = atomicCAS(&table[s].key, kEmpty, k);
      if (cur == kEmpty) { (*inserted)++; cur = k; }
    }
    if (cur == k) break;
    s = (s + 1) & mask;
    if (++probes > limit) { atomicExch(overflow, 1u); return false; }
  }
  *slot = s;
  return true;
}

// A row of those kernels, in front of and behind the kernel's own cache lookup.  row_without_lookup: the row's final id — a masked
// null (0), an encoded null or the all-ones key whose dedicated slot the prefix ranked —, kNoRow for a dedicated slot it did not rank
// (*s), or kLookup: the kernel's cache decides.  miss_row, for a row whose id is still kNoRow: a key the cache did not hold (probe)
// claims its slot in the insert table; the slot's first_row is lowered to this row, and the slot number, flagged with bit 31, is left
// for emit_kernel.  → false: overflow (claim_slot), the kernel returns.
__device__ __forceinline__ unsigned row_without_lookup(const InsertSide& t, bool ok, unsigned long long k, uint64_t* s) {
  *s = ok ? t.cap : t.cap + 1;   // the dedicated slot, should the row need one
  if (!ok) return t.encode_nulls ? t.null_id : 0u;  // masked null → index 0
  return k == kEmpty ? t.ones_id : kLookup;
}
__device__ __forceinline__ bool miss_row(Slot* __restrict__ table, uint64_t mask, unsigned* __restrict__ overflow, unsigned long long k, int64_t i, bool probe,
                                         uint64_t s, unsigned* fresh, unsigned* nmiss, unsigned* r) {
  if (probe && !claim_slot(k, table, mask, kProbeLimit, overflow, &s, fresh)) return false;
  if (table[s].first_row > (unsigned)i) atomicMin(&table[s].first_row, (unsigned)i);
  *r = 0x80000000u | (unsigned)s;
  (*nmiss)++;
  return true;
}

// ---- low cardinality: the prefix's keys in LDS ---------------------------------------------------
// When the 2^21-row prefix shows ≤ kSmallKeys distinct keys, their ids are already final (an id is the
// number of first occurrences before the key's own, and all of those lie in the prefix too).  The
// (key → id) pairs are copied into a kSmallSlots-entry open-addressing table that every workgroup of
// the main pass keeps in LDS: a hit costs no global access beyond the key load and the id store, so the
// pass runs at HBM speed instead of the L2 gather rate.  A miss (key not seen in the prefix) takes the
// global-table path and leaves a flagged slot number for emit_kernel.
constexpr int kSmallSlots = 8192;
constexpr int kSmallKeys = 4096;
constexpr int kSmallBlock = 1024;
constexpr int kSmallRows = 8;

__global__ __launch_bounds__(kBlock) void small_build_kernel(const Slot* __restrict__ table, uint64_t cap,
                                                              unsigned long long* __restrict__ skeys, unsigned* __restrict__ sids) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < cap; s += stride) {
    if (table[s].first_row == kNoRow) continue;
    const unsigned long long k = table[s].key;
    unsigned j = (unsigned)hash_int(k) & (kSmallSlots - 1);
    while (atomicCAS(&skeys[j], kEmpty, k) != kEmpty) j = (j + 1) & (kSmallSlots - 1);  // keys are distinct, ≤ half the entries
    sids[j] = table[s].id;
  }
}

__global__ __launch_bounds__(kSmallBlock) void insert_small_kernel(const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ valid,
                                                                    int64_t off, int64_t lo, int64_t hi, int encode_nulls, Slot* __restrict__ table,
                                                                    uint64_t cap, const unsigned long long* __restrict__ skeys,
                                                                    const unsigned* __restrict__ sids, unsigned* __restrict__ out_ids,
                                                                    unsigned long long* __restrict__ distinct, unsigned* __restrict__ overflow,
                                                                    unsigned long long* __restrict__ misses) {
  __shared__ unsigned long long l_keys[kSmallSlots];
  __shared__ unsigned l_ids[kSmallSlots];
  for (int j = threadIdx.x; j < kSmallSlots; j += kSmallBlock) { l_keys[j] = skeys[j]; l_ids[j] = sids[j]; }
  __syncthreads();
  const InsertSide side(table, cap, encode_nulls);
  const uint64_t mask = cap - 1;
  const int64_t stride = (int64_t)gridDim.x * kSmallBlock * kSmallRows;
  unsigned fresh = 0, nmiss = 0;
  // the next step's keys are requested before this step's are looked up: a lane has 2 × kSmallRows loads in flight and the
  // LDS work of one step hides behind the HBM latency of the next (one workgroup per CU: there is nobody else to hide it)
  unsigned long long kn[kSmallRows];
  bool okn[kSmallRows];
  auto fetch = [&](int64_t b) {
#pragma unroll
    for (int u = 0; u < kSmallRows; u++) {
      const int64_t i = b + (int64_t)u * kSmallBlock;
      okn[u] = i < hi && ah_bit(valid, off + i);
      kn[u] = okn[u] ? __builtin_nontemporal_load(&keys[i]) : 0ull;
    }
  };
  int64_t base = lo + (int64_t)blockIdx.x * kSmallBlock * kSmallRows + threadIdx.x;
  if (base < hi) fetch(base);
  for (; base < hi; base += stride) {
    unsigned long long k[kSmallRows];
    bool ok[kSmallRows];
#pragma unroll
    for (int u = 0; u < kSmallRows; u++) { k[u] = kn[u]; ok[u] = okn[u]; }
    if (base + stride < hi) fetch(base + stride);
    // first probes of all rows together (and the id that goes with a hit): eight independent LDS round trips, not a chain
    unsigned j0[kSmallRows], id0[kSmallRows];
    unsigned long long lk0[kSmallRows];
#pragma unroll
    for (int u = 0; u < kSmallRows; u++) {
      j0[u] = (unsigned)hash_int(k[u]) & (kSmallSlots - 1);
      lk0[u] = l_keys[j0[u]];
      id0[u] = l_ids[j0[u]];
    }
#pragma unroll
    for (int u = 0; u < kSmallRows; u++) {
      const int64_t i = base + (int64_t)u * kSmallBlock;
      if (i >= hi) break;
      uint64_t s;
      bool probe = false;
      unsigned r = row_without_lookup(side, ok[u], k[u], &s);   // final id, or kNoRow = "take the insert table with slot s"
      if (r == kLookup) {
        r = kNoRow;
        if (lk0[u] == k[u]) {
          r = id0[u];
        } else if (lk0[u] == kEmpty) {
          probe = true;
        } else {
          unsigned j = (j0[u] + 1) & (kSmallSlots - 1);
          for (;;) {
            const unsigned long long lk = l_keys[j];
            if (lk == k[u]) { r = l_ids[j]; break; }
            if (lk == kEmpty) { probe = true; break; }
            j = (j + 1) & (kSmallSlots - 1);
          }
        }
      }
      if (r == kNoRow && !miss_row(table, mask, overflow, k[u], i, probe, s, &fresh, &nmiss, &r)) return;
      if (out_ids) __builtin_nontemporal_store(r, &out_ids[i]);
    }
  }
  if (fresh) atomicAdd(distinct, (unsigned long long)fresh);
  if (nmiss) atomicAdd(misses, (unsigned long long)nmiss);
}

// ---- medium cardinality: the prefix's keys in a table sized for an XCD's L2 ---------------------------------
// The insert table is sized before anything is known about the column (2^22 slots = 64 MiB): 2^16 distinct keys sit
// there one per 64-byte line, 4 MiB of hot lines scattered over 64 MiB — PMC showed the main pass fetching a line
// from the fabric for every probe (35 B/row at 2^16 keys).  Once the prefix is ranked its (key → id) pairs are
// final, so they are re-packed into a read-only table at load ≤ ½ (2^16 keys: 2 MiB, 2^17: 4 MiB — one XCD's L2;
// beyond that still half the footprint in the Infinity Cache) and the main pass probes THAT: a hit costs one
// 16-byte load that stays in L2.  Misses take the insert table like in insert_small_kernel.
struct CSlot {
  unsigned long long key;
  unsigned id;
  unsigned pad;
};
__global__ __launch_bounds__(kBlock) void compact_build_kernel(const Slot* __restrict__ table, uint64_t cap, CSlot* __restrict__ ctab, uint64_t cmask) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (uint64_t s = (uint64_t)blockIdx.x * kBlock + threadIdx.x; s < cap; s += stride) {
    const SlotView v = load_slot(&table[s]);
    if (v.first_row == kNoRow) continue;
    uint64_t j = hash_int(v.key) & cmask;
    while (atomicCAS(&ctab[j].key, kEmpty, v.key) != kEmpty) j = (j + 1) & cmask;  // keys are distinct, load ≤ ½
    ctab[j].id = v.id;
  }
}

constexpr int kCompactRows = 8;  // rows per lane per step: eight independent probes in flight
__global__ __launch_bounds__(kBlock) void insert_compact_kernel(const unsigned long long* __restrict__ keys, const uint8_t* __restrict__ valid,
                                                                 int64_t off, int64_t lo, int64_t hi, int encode_nulls, Slot* __restrict__ table,
                                                                 uint64_t cap, const CSlot* __restrict__ ctab, uint64_t cmask,
                                                                 unsigned* __restrict__ out_ids, unsigned long long* __restrict__ distinct,
                                                                 unsigned* __restrict__ overflow, unsigned long long* __restrict__ misses) {
  const InsertSide side(table, cap, encode_nulls);
  const uint64_t mask = cap - 1;
  const int64_t stride = (int64_t)gridDim.x * kBlock * kCompactRows;
  unsigned fresh = 0, nmiss = 0;
  for (int64_t base = lo + (int64_t)blockIdx.x * kBlock * kCompactRows + threadIdx.x; base < hi; base += stride) {
    unsigned long long k[kCompactRows];
    bool ok[kCompactRows];
    uint4 cs[kCompactRows];
#pragma unroll
    for (int u = 0; u < kCompactRows; u++) {
      const int64_t i = base + (int64_t)u * kBlock;
      ok[u] = i < hi && ah_bit(valid, off + i);
      k[u] = ok[u] ? __builtin_nontemporal_load(&keys[i]) : 0ull;
    }
#pragma unroll
    for (int u = 0; u < kCompactRows; u++) cs[u] = *reinterpret_cast<const uint4*>(&ctab[hash_int(k[u]) & cmask]);
#pragma unroll
    for (int u = 0; u < kCompactRows; u++) {
      const int64_t i = base + (int64_t)u * kBlock;
      if (i >= hi) break;
      uint64_t s;
      bool probe = false;
      unsigned r = row_without_lookup(side, ok[u], k[u], &s);   // final id, or kNoRow = "take the insert table with slot s"
      if (r == kLookup) {
        r = kNoRow;
        uint64_t j = hash_int(k[u]) & cmask;
        uint4 c = cs[u];
        for (;;) {
          const unsigned long long ck = ((unsigned long long)c.y << 32) | c.x;
          if (ck == k[u]) { r = c.z; break; }
          if (ck == kEmpty) { probe = true; break; }
          j = (j + 1) & cmask;
          c = *reinterpret_cast<const uint4*>(&ctab[j]);
        }
      }
      if (r == kNoRow && !miss_row(table, mask, overflow, k[u], i, probe, s, &fresh, &nmiss, &r)) return;
      if (out_ids) __builtin_nontemporal_store(r, &out_ids[i]);
    }
  }
  if (fresh) atomicAdd(distinct, (unsigned long long)fresh);
  if (nmiss) atomicAdd(misses, (unsigned long long)nmiss);
}

static uint64_t next_pow2_u64(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// distinct keys expected among n rows when a prefix of p rows held d0 (uniform-urn model)
static double estimate_distinct(double d0, double p, double n) {
  const double r = d0 / p;
  if (r >= 0.999) return n;  // (almost) every prefix row was new: cannot tell, assume one key per row
  double lo = 1e-9, hi = 64.0;  // x = p / C;  g(x) = (1 − e^(−x)) / x falls from 1 to 0
  for (int it = 0; it < 60; it++) {
    const double mid = 0.5 * (lo + hi);
    if ((1.0 - exp(-mid)) / mid > r) lo = mid; else hi = mid;
  }
  const double C = p / (0.5 * (lo + hi));
  const double d = C * (1.0 - exp(-n / C));
  return d < n ? d : n;
}

struct EncodeResult {
  int64_t ndict;
  int32_t null_id;
};

// core: ids (optional, n int32), dict (optional), returns sizes.  Device pointers.
template <typename K>
int encode_core(ah_ctx* c, const K keys, const uint8_t* valid, int64_t off, int64_t n, int encode_nulls,
                int32_t* out_ids, uint64_t* out_dict, EncodeResult* res, int64_t* out_first_rows = nullptr, bool allow_partitioned = true) {
  res->ndict = 0;
  res->null_id = -1;
  if (n == 0) return AH_OK;
  // partition-first (ah_hash_part.hip) — forced by the option (tests, measurements); the automatic choice comes after the prefix below.
  // allow_partitioned = false: the caller's own temporaries live in the arena that path would take (the id-based group-by)
  auto try_partitioned = [&](int lp, bool* done, int slots2 = 4096) -> int {
    *done = false;
    if constexpr (K::kLdsTable) {
      int used = 0;
      int64_t nd = 0;
      int32_t nid = -1;
      int prc = lp <= 10 ? ah_encode_partitioned_try(c, (const uint64_t*)keys.keys, valid, off, n, encode_nulls, lp, c->opt_encode_part_slots == 4096 ? 4096 : 8192, out_ids, out_dict, out_first_rows, &nd, &nid, &used)
                         : ah_encode_partitioned2_try(c, (const uint64_t*)keys.keys, valid, off, n, encode_nulls, lp, slots2, out_ids, out_dict, out_first_rows, &nd, &nid, &used);
      if (prc != AH_OK) return prc;
      if (used) { res->ndict = nd; res->null_id = nid; *done = true; }
    }
    return AH_OK;
  };
  if (K::kLdsTable && allow_partitioned && c->opt_encode_partition >= 3) {
    bool done;
    int prc = try_partitioned(c->opt_encode_partition > 13 ? 13 : c->opt_encode_partition, &done);
    if (prc != AH_OK || done) return prc;
  }
  // slot numbers travel through the int32 id column: the largest table (2n slots + 2) must stay below 2^32 − 1
  if (n > ((int64_t)1 << 30)) return ah_fail(c, AH_ENOTIMPL, "hash: more than 2^30 rows per call");
  // the first look's verdict, from the distinct keys d16 among the first 2^16 rows: partitions (and how many), or *undecided (almost every
  // row was new: the 2^21-row prefix will tell), or neither (the global table).  → AH_OK with *done = true when the partitions answered.
  auto decide_after_look = [&](double d16, bool overflowed, bool* undecided, bool* done, bool* attempted) -> int {
    const double hi = (double)((int64_t)1 << 16);
    *done = false;
    *attempted = false;
    const double est = estimate_distinct(d16, hi, (double)n);
    // (almost) every one of the 2^16 rows was new: ≥ 2^25 keys or so, too few repeats to say how many — the prefix below will tell
    *undecided = !overflowed && d16 >= 0.999 * hi;
    if (overflowed || est < (double)c->opt_encode_part_min || est > 8192.0 * 4400.0) return AH_OK;
    int lp = 8;   // 256 … 1024 partitions of ≤ 4400 expected keys in one cut (8192-slot tables); beyond, two cuts into 2048 … 8192 of ≤ 2200 (4096-slot tables)
    const double kpp1 = c->opt_encode_part_slots == 4096 ? 2200.0 : 4400.0;
    while (lp < 10 && est / (double)(1 << lp) > kpp1) lp++;
    int slots2 = 4096;
    if (est / (double)(1 << lp) > kpp1) {
      lp = 11;
      while (lp < 13 && est / (double)(1 << lp) > 2200.0) lp++;
      // 21 … 36 M keys: 8192 partitions with the large tables.  (The small ones take 3072 keys; 2600 expected leaves room for the
      // estimate's ± 9 % at this cardinality — 128 repeats among the 2^16 sampled rows — and the partitions' own spread.)
      if (est / (double)(1 << lp) > 2600.0) slots2 = 8192;
    }
    *attempted = true;
    return try_partitioned(lp, done, slots2);
  };
  // Large calls look BEFORE anything is spent on the global table (ah_encode_first_look: one launch, ≈ 25 µs, against ≈ 90 µs of table
  // fill + staged inserts + polled read): a call the partitions answer never touches the table.  Small calls (n < 2^24) keep the look
  // that falls out of the staged inserts — it costs them nothing, and this one would cost a launch and a wait on every call.
  bool looked = false, look_undecided = false;
  if constexpr (K::kLdsTable) if (allow_partitioned && c->opt_encode_partition == 1 && n >= ((int64_t)1 << 24) && c->opt_encode_early_look) {
    uint64_t d16 = 0;
    int lrc = ah_encode_first_look(c, (const uint64_t*)keys.keys, valid, off, (int64_t)1 << 16, &d16);
    if (lrc != AH_OK) return lrc;
    bool done = false, attempted = false;
    lrc = decide_after_look((double)d16, false, &look_undecided, &done, &attempted);
    if (lrc != AH_OK || done) return lrc;
    looked = true;   // (a void attempt left no slot numbers behind: the table has not been touched yet)
  }
  const int64_t nwords = ah_ceil_div(n, 64);
  const int64_t ntiles = ah_ceil_div(nwords, 32);
  const uint64_t cap_max = next_pow2_u64((uint64_t)n * 2 < 64 ? 64 : (uint64_t)n * 2);
  uint64_t cap = cap_max < ((uint64_t)1 << 22) ? cap_max : ((uint64_t)1 << 22);
  unsigned long long* distinct = (unsigned long long*)&c->dscalars[4];
  unsigned* overflow = (unsigned*)&c->dscalars[5];
  unsigned long long* total = (unsigned long long*)&c->dscalars[6];
  int* null_id = (int*)&c->dscalars[7];
  unsigned long long* misses = (unsigned long long*)&c->dscalars[8];
  // tunable, for measurements: 0 = plain (ids in a separate pass), 1 = direct ids, 2 (default) = direct ids + LDS table
  const int direct_path = c->opt_hash_direct;
  bool resized = false;  // the table was re-planned: it is large and the prefix holds a minority of its keys
  for (;;) {
    // scratch: table | firsts | wordprefix | tilecnt | tileoff
    size_t table_bytes = (size_t)(cap + 2) * sizeof(Slot);
    size_t firsts_bytes = (size_t)nwords * 8;
    size_t wp_bytes = ((size_t)nwords * 4 + 7) & ~(size_t)7;
    size_t tc_bytes = ((size_t)ntiles * 4 + 7) & ~(size_t)7;
    size_t to_bytes = (size_t)ntiles * 8;
    void* scratch;
    const size_t small_bytes = (size_t)kSmallSlots * 12;
    const size_t compact_bytes = K::kLdsTable ? (size_t)(cap / 2) * sizeof(CSlot) : 0;  // ≤ cap/4 prefix keys at load ≤ ½
    int rc = ah_scratch_reserve(c, table_bytes + firsts_bytes + wp_bytes + tc_bytes + to_bytes + small_bytes + compact_bytes + 64, &scratch);
    if (rc != AH_OK) return rc;
    Slot* table = (Slot*)scratch;
    unsigned long long* firsts = (unsigned long long*)((uint8_t*)scratch + table_bytes);
    unsigned* wordprefix = (unsigned*)((uint8_t*)firsts + firsts_bytes);
    int* tilecnt = (int*)((uint8_t*)wordprefix + wp_bytes);
    int64_t* tileoff = (int64_t*)((uint8_t*)tilecnt + tc_bytes);
    unsigned long long* skeys = (unsigned long long*)((uint8_t*)tileoff + to_bytes);
    unsigned* sids = (unsigned*)(skeys + kSmallSlots);
    CSlot* ctab = (CSlot*)(((uintptr_t)(sids + kSmallSlots) + 63) & ~(uintptr_t)63);

    AH_HIP(c, hipMemsetAsync(table, 0xFF, table_bytes, c->stream));
    AH_HIP(c, hipMemsetAsync(&c->dscalars[4], 0, 3 * sizeof(uint64_t), c->stream));
    AH_HIP(c, hipMemsetAsync(null_id, 0xFF, sizeof(uint64_t), c->stream));
    // Capacity planning without a wasted pass: insert a PREFIX of the rows first and look at
    // how many distinct keys it produced.  Low-cardinality columns (the common case) just carry
    // on into the same table; a prefix that already fills a quarter of the table means the
    // column needs a table sized from the extrapolated distinct count — restart with that.
    const int64_t prefix = n < ((int64_t)1 << 21) ? n : ((int64_t)1 << 21);
    unsigned grid = ah_stream_grid(c, ah_ceil_div(n, (int64_t)kBlock * kInsertRows));  // emit_kernel: 4 rows per lane as well
    // staged: with every prefix row in flight at once against an empty table, a low-cardinality column turns
    // into millions of CAS / atomicMin on a few addresses (200 µs for 1024 keys).  A few thousand rows first,
    // then the rest mostly finds settled slots and issues no atomics at all.
    bool part_undecided = false;
    // A partition-first attempt that voids itself (a partition's table overflowed: the head of the column misled the estimate)
    // has already sent ids home — over the slot numbers this path keeps in out_ids for the rows it has inserted.  Put them
    // back: every key of those rows sits in the table, so the second insert only probes (no claim, no counter moves).
    auto restore_slot_numbers = [&](int64_t rows) -> int {
      if (!out_ids || rows <= 0) return AH_OK;
      insert_kernel<K><<<ah_stream_grid(c, ah_ceil_div(rows, (int64_t)kBlock * kInsertRows)), kBlock, 0, c->stream>>>(
          keys, valid, off, 0, rows, encode_nulls, table, cap, (unsigned*)out_ids, 0u, 0u, distinct, overflow, misses);
      AH_LAUNCH_CHECK(c);
      return AH_OK;
    };
    {
      int64_t lo = 0;
      for (int64_t hi : {(int64_t)1 << 12, (int64_t)1 << 16, prefix}) {
        if (hi > prefix) hi = prefix;
        if (hi <= lo) continue;
        unsigned g = ah_stream_grid(c, ah_ceil_div(hi - lo, (int64_t)kBlock * kInsertRows));
        insert_kernel<K><<<g, kBlock, 0, c->stream>>>(keys, valid, off, lo, hi, encode_nulls, table, cap,
                                                   (unsigned*)out_ids, 0u, 0u, distinct, overflow, misses);
        AH_LAUNCH_CHECK(c);
        lo = hi;
        if (K::kLdsTable && allow_partitioned && c->opt_encode_partition == 1 && !resized && !looked && hi == ((int64_t)1 << 16) && n >= ((int64_t)1 << 22)) {
          // A first look after 2^16 rows: ≈ 3·10^5 … 4.5·10^6 expected keys are more than the LDS / re-packed tables and the caches
          // hold — cut the rows by key hash and give every partition a table in LDS (ah_hash_part.hip; ≤ 4400 expected keys per
          // partition of 256 … 1024).  2^16 rows show 2^19 evenly drawn keys with ≈ 3900 repeats (± 62): the urn model's estimate
          // is good to a few per cent up to 2^22 keys; a column whose head misleads (sorted keys) is caught by the partition
          // pass itself (a table that overflows voids the attempt) or simply stays on this path.
          unsigned long long look[2];   // {distinct so far, overflow flag}: polled, not synchronised — this look is on every large call's path
          if ((rc = ah_mailbox_read(c, (const unsigned long long*)&c->dscalars[4], 2, look)) != AH_OK) return rc;
          c->pinned[0] = look[0]; c->pinned[1] = look[1];
          bool done, attempted;
          int prc = decide_after_look((double)look[0], (unsigned)look[1] != 0, &part_undecided, &done, &attempted);
          if (prc != AH_OK || done) return prc;
          if (attempted && (prc = restore_slot_numbers(hi)) != AH_OK) return prc;
        }
      }
    }
    if (looked && !resized) part_undecided = look_undecided;
    bool restart = false, small = false, direct = false, compact = false;
    uint64_t d0 = 0;
    if (prefix < n && cap < cap_max) {
      if ((rc = ah_mailbox_read(c, (const unsigned long long*)&c->dscalars[4], 2, (unsigned long long*)c->pinned)) != AH_OK) return rc;
      d0 = *(volatile uint64_t*)&c->pinned[0];
      bool ovf = *(volatile unsigned*)&c->pinned[1] != 0;
      if (part_undecided && !ovf) {   // 2^21 rows hold enough repeats to tell 2^25 keys from 2^26: up to ≈ 36 M expected keys take the two-cut path
        const double est = estimate_distinct((double)d0, (double)prefix, (double)n);
        if (est <= 8192.0 * 4400.0) {
          bool done;
          int prc = try_partitioned(13, &done, est / 8192.0 > 2600.0 ? 8192 : 4096);
          if (prc != AH_OK || done) return prc;
          if ((prc = restore_slot_numbers(prefix)) != AH_OK) return prc;
        }
      }
      if (ovf || d0 > cap / 4) {
        // extrapolate with the urn model (keys drawn uniformly from C values show d0 = C·(1 − e^(−p/C))
        // distinct ones in a prefix of p rows): solve for C, predict the distinct count of all n rows,
        // size for load ≤ ⅓.  A skewed column has more distinct keys than this predicts; the probe
        // limit then trips and the insert is redone with 16× the slots (results never depend on it).
        uint64_t want = next_pow2_u64((uint64_t)(estimate_distinct((double)d0, (double)prefix, (double)n) * 3.0) + 64);
        if (want < cap * 4) want = cap * 4;
        cap = want < cap_max ? want : cap_max;
        restart = true;
        resized = true;
      }
      direct = !restart && !ovf && !resized && direct_path;
      small = K::kLdsTable && direct && d0 <= (uint64_t)kSmallKeys && direct_path > 1;
      compact = K::kLdsTable && direct && !small && direct_path > 1 && direct_path != 3;   // 3: measurement switch, no re-packed table
    }
    if (restart) continue;
    // first-seen ranks of the used slots over the first `rows` rows: table[].id, dict, first_rows, total, null_id
    auto rank_slots = [&](int64_t rows) -> int {
      const int64_t nw = ah_ceil_div(rows, 64), nt = rank_tiles(nw);
      AH_HIP(c, hipMemsetAsync(firsts, 0, (size_t)nw * 8, c->stream));
      mark_kernel<<<ah_stream_grid(c, ah_ceil_div((int64_t)cap + 2, kBlock)), kBlock, 0, c->stream>>>(table, cap + 2, firsts);
      AH_LAUNCH_CHECK(c);
      word_prefix_kernel<<<(unsigned)ah_ceil_div(nw, kBlock), kBlock, 0, c->stream>>>(firsts, nw, wordprefix, tilecnt);
      AH_LAUNCH_CHECK(c);
      scan_kernel<<<1, 1024, 0, c->stream>>>(tilecnt, nt, tileoff, total);
      AH_LAUNCH_CHECK(c);
      assign_kernel<<<ah_stream_grid(c, ah_ceil_div((int64_t)cap + 2, kBlock)), kBlock, 0, c->stream>>>(
          table, cap, firsts, wordprefix, tileoff, (unsigned long long*)out_dict, null_id, (long long*)out_first_rows);
      AH_LAUNCH_CHECK(c);
      return AH_OK;
    };
    // Rows after the prefix: the prefix's keys are ranked first (their ids are final: an id is the number
    // of first occurrences before the key's own, all of which lie in the prefix too), so the main pass can
    // write ids directly — out of LDS when the prefix has ≤ kSmallKeys keys, else out of the slot it probes
    // anyway — and only rows with a key the prefix did not have ("misses") wait for emit_kernel.  Not done
    // after a restart: that table is large (ranking scans it) and most of its keys are still to come.
    int64_t direct_from = n;  // rows from here on hold final ids or flagged slot numbers
    bool ranked = false;      // table[].id, dict, first_rows, total are final
    if (direct) {
      if ((rc = rank_slots(prefix)) != AH_OK) return rc;
      AH_HIP(c, hipMemsetAsync(misses, 0, 8, c->stream));
      direct_from = prefix;
      int64_t lo = prefix;
      if constexpr (K::kLdsTable) if (small) {
        AH_HIP(c, hipMemsetAsync(skeys, 0xFF, (size_t)kSmallSlots * 8, c->stream));
        small_build_kernel<<<ah_stream_grid(c, ah_ceil_div((int64_t)cap, kBlock)), kBlock, 0, c->stream>>>(table, cap, skeys, sids);
        AH_LAUNCH_CHECK(c);
        // a probe segment first: a column whose later rows keep bringing new keys (sorted keys, say)
        // misses the LDS table all the time and is better served by the plain kernel
        const int64_t probe_end = n - prefix > ((int64_t)1 << 23) ? prefix + ((int64_t)1 << 22) : n;
        const unsigned sgrid = (unsigned)c->num_cu;
        insert_small_kernel<<<sgrid, kSmallBlock, 0, c->stream>>>(keys.keys, valid, off, prefix, probe_end, encode_nulls,
                                                                  table, cap, skeys, sids, (unsigned*)out_ids, distinct, overflow, misses);
        AH_LAUNCH_CHECK(c);
        lo = probe_end;
        if (probe_end < n) {
          if ((rc = ah_mailbox_read(c, misses, 1, (unsigned long long*)c->pinned)) != AH_OK) return rc;
          if (*(volatile uint64_t*)c->pinned * 8 < (uint64_t)(probe_end - prefix)) {
            insert_small_kernel<<<sgrid, kSmallBlock, 0, c->stream>>>(keys.keys, valid, off, probe_end, n, encode_nulls,
                                                                      table, cap, skeys, sids, (unsigned*)out_ids, distinct, overflow, misses);
            AH_LAUNCH_CHECK(c);
            lo = n;
          }
        }
      }
      if constexpr (K::kLdsTable) if (compact && lo < n) {
        const uint64_t ccap = next_pow2_u64(d0 * 2 < 64 ? 64 : d0 * 2);
        AH_HIP(c, hipMemsetAsync(ctab, 0xFF, (size_t)ccap * sizeof(CSlot), c->stream));
        compact_build_kernel<<<ah_stream_grid(c, ah_ceil_div((int64_t)cap, kBlock)), kBlock, 0, c->stream>>>(table, cap, ctab, ccap - 1);
        AH_LAUNCH_CHECK(c);
        // a probe segment first, as above: a miss costs a second, dependent walk (re-packed table, then the insert table), so a
        // column that keeps bringing keys the prefix did not hold (2^20 uniform keys: 14 % of the rows; Zipf tails) is
        // better served by the plain kernel, whose first probes are all in flight together — measured 1.4 → 2.1 ms otherwise
        const int64_t seg_lo = lo, probe_end = n - lo > ((int64_t)1 << 23) ? lo + ((int64_t)1 << 22) : n;
        insert_compact_kernel<<<ah_stream_grid(c, ah_ceil_div(probe_end - lo, (int64_t)kBlock * kCompactRows)), kBlock, 0, c->stream>>>(
            keys.keys, valid, off, lo, probe_end, encode_nulls, table, cap, ctab, ccap - 1, (unsigned*)out_ids, distinct, overflow, misses);
        AH_LAUNCH_CHECK(c);
        lo = probe_end;
        if (probe_end < n) {
          if ((rc = ah_mailbox_read(c, misses, 1, (unsigned long long*)c->pinned)) != AH_OK) return rc;
          if (*(volatile uint64_t*)c->pinned * 64 < (uint64_t)(probe_end - seg_lo)) {
            insert_compact_kernel<<<ah_stream_grid(c, ah_ceil_div(n - lo, (int64_t)kBlock * kCompactRows)), kBlock, 0, c->stream>>>(
                keys.keys, valid, off, lo, n, encode_nulls, table, cap, ctab, ccap - 1, (unsigned*)out_ids, distinct, overflow, misses);
            AH_LAUNCH_CHECK(c);
            lo = n;
          }
        }
      }
      if (lo < n) {
        insert_kernel<K><<<grid, kBlock, 0, c->stream>>>(keys, valid, off, lo, n, encode_nulls, table, cap,
                                                      (unsigned*)out_ids, 0x80000000u, (unsigned)prefix, distinct, overflow, misses);
        AH_LAUNCH_CHECK(c);
      }
      {   // dscalars[4 … 8] = distinct, overflow, total, null id, misses: one polled read
        unsigned long long w5[5];
        if ((rc = ah_mailbox_read(c, (const unsigned long long*)&c->dscalars[4], 5, w5)) != AH_OK) return rc;
        c->pinned[0] = w5[4]; c->pinned[1] = w5[1];
      }
      ranked = *(volatile uint64_t*)&c->pinned[0] == 0 && *(volatile unsigned*)&c->pinned[1] == 0;
      *(volatile uint64_t*)c->pinned = *(volatile uint64_t*)&c->pinned[1];  // overflow flag where the check below reads it
    } else {
      if (prefix < n) {
        insert_kernel<K><<<grid, kBlock, 0, c->stream>>>(keys, valid, off, prefix, n, encode_nulls, table, cap,
                                                      (unsigned*)out_ids, 0u, 0u, distinct, overflow, misses);
        AH_LAUNCH_CHECK(c);
      }
      if ((rc = ah_mailbox_read(c, (const unsigned long long*)overflow, 1, (unsigned long long*)c->pinned)) != AH_OK) return rc;
    }
    if (*(volatile unsigned*)c->pinned) {
      if (cap >= cap_max) return ah_fail(c, AH_EINVALID, "hash: table overflow at maximum capacity (internal error)");
      cap = cap * 16 < cap_max ? cap * 16 : cap_max;
      resized = true;
      continue;
    }
    if (!ranked && (rc = rank_slots(n)) != AH_OK) return rc;
    if (out_ids) {
      // no miss: only the prefix rows still hold slot numbers
      const int64_t rows = ranked ? prefix : n;
      emit_kernel<<<ah_stream_grid(c, ah_ceil_div(rows, (int64_t)kBlock * 4)), kBlock, 0, c->stream>>>(table, out_ids, rows, direct_from);
      AH_LAUNCH_CHECK(c);
    }
    if ((rc = ah_mailbox_read(c, (const unsigned long long*)&c->dscalars[6], 2, (unsigned long long*)c->pinned)) != AH_OK) return rc;
    res->ndict = (int64_t) * (volatile uint64_t*)&c->pinned[0];
    res->null_id = *(volatile int32_t*)&c->pinned[1];
    return AH_OK;
  }
}

}  // namespace

// the ids of the id-based group-by (ah_hash_agg.hip): nulls are a group, and the partition-first encode is not tried — the caller's own
// temporaries live in the arena that path would take
int ah_encode_u64_groups(ah_ctx* c, const uint64_t* keys, const uint8_t* kvalid, int64_t koff, int64_t n, int32_t* ids, uint64_t* out_keys,
                         int64_t* out_first_rows, int64_t* out_ngroups, int32_t* out_null_group) {
  EncodeResult res;
  int rc = encode_core(c, U64Keys{(const unsigned long long*)keys}, kvalid, koff, n, /*encode_nulls=*/1, ids, out_keys, &res, out_first_rows, /*allow_partitioned=*/false);
  if (rc != AH_OK) return rc;
  *out_ngroups = res.ndict;
  *out_null_group = res.null_id;
  return AH_OK;
}

// the ids of ah_group_ids (ah_group_keys.hip) over ONE column of 8-byte words — a key column as it is, or the packed column of a
// narrow tuple: nulls are a group, and every route is open (LDS tables, first look, partition-first) — the caller keeps nothing in
// the scratch or temp arena
int ah_encode_u64_first_seen(ah_ctx* c, const uint64_t* keys, const uint8_t* valid, int64_t off, int64_t n, int32_t* ids, int64_t* out_first_rows,
                             int64_t* out_ngroups) {
  EncodeResult res;
  int rc = encode_core(c, U64Keys{(const unsigned long long*)keys}, valid, off, n, /*encode_nulls=*/1, ids, nullptr, &res, out_first_rows);
  if (rc != AH_OK) return rc;
  *out_ngroups = res.ndict;
  return AH_OK;
}

// … and over a tuple of columns the caller has checked (2 … 8 of them): the global table with TupleKeys.  A null is a value of its
// column, so the table sees no validity of its own.
int ah_encode_tuple_first_seen(ah_ctx* c, int ncols, const ah_group_key* keys, int64_t n, int32_t* ids, int64_t* out_first_rows, int64_t* out_ngroups) {
  KeyCol cols[8];
  for (int j = 0; j < 8; j++) {
    cols[j] = KeyCol{nullptr, nullptr, nullptr, 0, kColNone, 0};
    if (j >= ncols) continue;
    const ah_group_key& k = keys[j];
    if (k.offset_width == 4) cols[j] = KeyCol{(const int32_t*)k.offsets + k.off, k.data, k.valid, k.off, kColVar4, 0};
    else if (k.offset_width == 8) cols[j] = KeyCol{(const long long*)k.offsets + k.off, k.data, k.valid, k.off, kColVar8, 0};
    else if (k.bits) cols[j] = KeyCol{nullptr, k.data, k.valid, k.off, kColBits, 0};
    else cols[j] = KeyCol{nullptr, k.data + k.off * (int64_t)k.byte_width, k.valid, k.off, kColFixed, k.byte_width};
  }
  EncodeResult res;
  int rc;
  auto run = [&](auto keys_of) { rc = encode_core(c, keys_of, nullptr, 0, n, /*encode_nulls=*/1, ids, nullptr, &res, out_first_rows); };
  if (ncols <= 2) { TupleKeys<2> t; for (int j = 0; j < 2; j++) t.col[j] = cols[j]; run(t); }
  else if (ncols <= 4) { TupleKeys<4> t; for (int j = 0; j < 4; j++) t.col[j] = cols[j]; run(t); }
  else { TupleKeys<8> t; for (int j = 0; j < 8; j++) t.col[j] = cols[j]; run(t); }
  if (rc != AH_OK) return rc;
  *out_ngroups = res.ndict;
  return AH_OK;
}

// what the three encode exports end with: the validity of the indices, then the sizes
static int encode_finish(ah_ctx* c, const EncodeResult& res, const uint8_t* valid, int64_t off, int64_t n, int encode_nulls, uint8_t* out_ids_valid,
                         int64_t* out_ndict_host, int32_t* out_null_id_host) {
  if (out_ids_valid) {
    // indices validity: all set when nulls are encoded (or there is no validity);
    // otherwise the input validity (NullEncodingMask, vector_hash.go:224-230)
    // the bitmap is this call's to define up to its last byte: the bits behind row n − 1 are zero (ah_copy_bitmap and ah_set_bits_to keep
    // what lies outside their range — right for an executor's slice, wrong for a fresh output whose memory held something else before)
    AH_HIP(c, hipMemsetAsync(out_ids_valid, 0, (size_t)((n + 7) / 8), c->stream));
    int rc = valid && !encode_nulls ? ah_copy_bitmap(c, valid, off, n, out_ids_valid, 0, 0) : ah_set_bits_to(c, out_ids_valid, 0, n, 1);
    if (rc != AH_OK) return rc;
    AH_HIP(c, hipStreamSynchronize(c->stream));
  }
  if (out_ndict_host) *out_ndict_host = res.ndict;
  if (out_null_id_host) *out_null_id_host = res.null_id;
  return AH_OK;
}

AH_EXPORT int ah_hash_binary_encode(ah_ctx* c, int offset_width, const void* offsets, const uint8_t* data, const uint8_t* valid, int64_t off,
                                    int64_t n, int encode_nulls, int32_t* out_ids, uint8_t* out_ids_valid, int64_t* out_first_rows,
                                    int64_t* out_ndict_host, int32_t* out_null_id_host) {
  AH_ENTER(c);
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "hash: negative length/offset");
  if (offset_width != 4 && offset_width != 8) return ah_fail(c, AH_EINVALID, "hash: offset width must be 4 or 8");
  if (out_ndict_host) *out_ndict_host = 0;
  if (out_null_id_host) *out_null_id_host = -1;
  if (n == 0) return AH_OK;
  if (!offsets || !out_first_rows) return ah_fail(c, AH_EINVALID, "hash: null buffer");
  if ((uintptr_t)offsets & (uintptr_t)(offset_width - 1)) return ah_fail(c, AH_EINVALID, "hash: offsets not element-aligned");
  EncodeResult res;
  int rc = offset_width == 4
               ? encode_core(c, ByteKeys<4>{byte_rows(4, offsets, data, 0, off)}, valid, off, n, encode_nulls, out_ids, nullptr, &res, out_first_rows)
               : encode_core(c, ByteKeys<8>{byte_rows(8, offsets, data, 0, off)}, valid, off, n, encode_nulls, out_ids, nullptr, &res, out_first_rows);
  if (rc != AH_OK) return rc;
  return encode_finish(c, res, valid, off, n, encode_nulls, out_ids_valid, out_ndict_host, out_null_id_host);
}

AH_EXPORT int ah_hash_fixed_encode(ah_ctx* c, int byte_width, const uint8_t* data, const uint8_t* valid, int64_t off, int64_t n, int encode_nulls,
                                   int32_t* out_ids, uint8_t* out_ids_valid, int64_t* out_first_rows, uint8_t* out_dict, int64_t* out_ndict_host,
                                   int32_t* out_null_id_host) {
  AH_ENTER(c);
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "hash: negative length/offset");
  if (byte_width < 1 || byte_width > 4096) return ah_fail(c, AH_EINVALID, "hash: fixed width must be 1..4096 bytes");
  if (out_ndict_host) *out_ndict_host = 0;
  if (out_null_id_host) *out_null_id_host = -1;
  if (n == 0) return AH_OK;
  if (!data || !out_first_rows) return ah_fail(c, AH_EINVALID, "hash: null buffer");
  EncodeResult res;
  int rc = encode_core(c, ByteKeys<0>{byte_rows(0, nullptr, data, byte_width, off)}, valid, off, n, encode_nulls, out_ids, nullptr, &res, out_first_rows);
  if (rc != AH_OK) return rc;
  if (out_dict && res.ndict > 0) {
    fixed_dict_kernel<<<ah_stream_grid(c, ah_ceil_div(res.ndict * byte_width, kBlock), 8), kBlock, 0, c->stream>>>(data + off * (int64_t)byte_width, byte_width,
                                                                                                                    (const long long*)out_first_rows, res.ndict, res.null_id, out_dict);
    AH_LAUNCH_CHECK(c);
    AH_HIP(c, hipStreamSynchronize(c->stream));
  }
  return encode_finish(c, res, valid, off, n, encode_nulls, out_ids_valid, out_ndict_host, out_null_id_host);
}

AH_EXPORT int ah_hash_u64_encode(ah_ctx* c, const uint64_t* keys, const uint8_t* valid, int64_t off, int64_t n,
                                 int encode_nulls, int32_t* out_ids, uint8_t* out_ids_valid, uint64_t* out_dict,
                                 int64_t* out_ndict_host, int32_t* out_null_id_host) {
  AH_ENTER(c);
  if (n < 0 || off < 0) return ah_fail(c, AH_EINVALID, "hash: negative length/offset");
  if (out_ndict_host) *out_ndict_host = 0;
  if (out_null_id_host) *out_null_id_host = -1;
  if (n == 0) return AH_OK;
  if (!keys) return ah_fail(c, AH_EINVALID, "hash: null keys");
  EncodeResult res;
  int rc = encode_core(c, U64Keys{(const unsigned long long*)keys}, valid, off, n, encode_nulls, out_ids, out_dict, &res);
  if (rc != AH_OK) return rc;
  return encode_finish(c, res, valid, off, n, encode_nulls, out_ids_valid, out_ndict_host, out_null_id_host);
}

// ---- key → owner partition for the multi-GPU merge (SURVEY.md §8e plan A) ----------------------
// owner = (hashInt(key) >> 40) mod nparts, hashInt as in internal/hashing/hash_funcs.go:60-67: every
// rank computes the same owner for a key, so partial groups of one key all meet on one GPU.
namespace {
__global__ __launch_bounds__(kBlock) void partition_kernel(const unsigned long long* __restrict__ keys, int64_t n, unsigned nparts,
                                                            int32_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) out[i] = (int32_t)((hash_int(keys[i]) >> 40) % nparts);
}
}  // namespace

AH_EXPORT int ah_hash_partition_u64(ah_ctx* c, const uint64_t* keys, int64_t n, int nparts, int32_t* out_part) {
  AH_ENTER(c);
  if (n < 0 || nparts < 1) return ah_fail(c, AH_EINVALID, "hash_partition: bad length / partition count");
  if (n == 0) return AH_OK;
  if (!keys || !out_part) return ah_fail(c, AH_EINVALID, "hash_partition: null buffer");
  partition_kernel<<<ah_stream_grid(c, ah_ceil_div(n, kBlock), 8), kBlock, 0, c->stream>>>((const unsigned long long*)keys, n, (unsigned)nparts, out_part);
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}
