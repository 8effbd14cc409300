// ah_sort_binary.hip — sort_indices by Binary / String, LargeBinary / LargeString, FixedSizeBinary and Decimal128 / 256 keys.
//
// Replaces the comparators kernels.SortIndices uses for these types (arrow/compute/internal/kernels/vector_sort.go:195-245:
// bytes.Compare on the values, decimal128.Num.Cmp / decimal256.Num.Cmp) under the same stable partition + SortStableFunc as
// the numeric keys (ah_sort.hip): nulls to the end or the start in input order, no NaN category, descending reverses the
// values and keeps ties in input order.  Binary and fixed-size binary values order bytewise, unsigned, a proper prefix first
// ("ab" < "ab\0" < "abc"); decimals by signed value (their storage is little-endian two's complement, so not bytewise).
//
// A key is one more stable sort of the current row order with the contract of sort_by_column: it reorders rows_in (or the
// input order) and leaves the new order in b.ra, so it mixes with numeric keys in any position of a multi-key sort.
//
// MSD refinement over 64-bit chunks of the value.  Round r maps every row to a 64-bit key:
//   var-length: bytes [7r, 7r + 7) big-endian in the top 7 bytes, zero-padded, and min(remaining length, 8) in the low byte —
//               that byte puts "ab" (2) before "ab\0" (3), and a row is still undecided after the round only while it is 8;
//   fixed-size: bytes [8r, 8r + 8) big-endian, zero-padded; rows continue until the width is used up;
//   decimal:    word (words − 1 − r), most significant first, the sign bit of the top word flipped;
// complemented for descending.  A row's bytes are found through ah_bytes.h's ByteRows (layout chosen at run time).  Values are
// read with aligned 8-byte loads and a funnel shift (load_le): a load is issued only for an aligned word that holds at least one
// byte of the value, so no read leaves the pages of the value's bytes.
//   round 0: one stable partition pass (null / rest, respecting rows_in) creates (key, row) pairs, then the stable LSD passes
//            of ah_sort_radix.h over the key bytes that vary — the numeric sort with a different key;
//   then:    the runs of equal, continuing keys are the rows still tied.  A flag scan compacts their positions in b.ra and
//            marks where each run starts; only those rows get the next round's key and are re-sorted inside their run,
//            stably by their current position: runs of ≤ kWaveSeg rows by one wave each (bitonic network over (key,
//            position in the run) in LDS), otherwise all tied rows of the round by stable LSD passes over (key, run index).
//            The sorted rows are written back into their run.  The rounds stop when no run continues.
// Traffic: round 0 costs what an Int64 sort of the same rows costs plus the offsets / data reads (≈ 16 + 8-16 B/row); a later
// round costs ≈ 120 B per tied row (keys 50, flag scan + compaction 50, run starts 16) + 32 B per LSD pass when a run is
// large.  The number of rounds is the longest common prefix among tied values / 7: the worst case is many copies of one long
// value (every row tied in every round, L / 7 rounds of ≈ 120 B/row plus two read-backs each; no LSD pass runs, because
// neither the key nor the run index varies).
#include "ah_sort_radix.h"
#include "ah_bytes.h"

namespace {

constexpr int kWaveSeg = 512;  // longest run the one-wave bitonic network sorts
enum { kVar = 0, kFixed = 1, kDecimal = 2 };

struct BinDesc {
  int kind, ow, nrounds, descending;  // ow: the offset width of a var-length key, 0 for a fixed-width one
  ByteRows rows;                      // of row 0 of the column (ah_bytes.h)
  const uint8_t* valid;
  int64_t off;                        // validity bit off + row
};

// nb ≤ 8 bytes at p, byte 0 in the low bits, zeros above nb; only aligned words holding a byte of [p, p + nb) are loaded
__device__ __forceinline__ unsigned long long load_le(const uint8_t* p, int nb) {
  if (nb <= 0) return 0ull;
  const uintptr_t a = (uintptr_t)p;
  const int sh = (int)(a & 7);
  const unsigned long long* w = (const unsigned long long*)(a - sh);
  unsigned long long v = w[0] >> (8 * sh);
  if (sh + nb > 8) v |= w[1] << (64 - 8 * sh);  // sh ≥ 1 here
  if (nb < 8) v &= (1ull << (8 * nb)) - 1;
  return v;
}

__device__ __forceinline__ unsigned long long bin_key(const BinDesc& d, unsigned row, int r) {
  const uint8_t* p;
  int64_t len;
  row_at(d.ow, d.rows, row, &p, &len);
  unsigned long long k;
  if (d.kind == kVar) {
    const int64_t rem = len - 7 * (int64_t)r;
    const int nb = rem < 7 ? (rem > 0 ? (int)rem : 0) : 7;
    k = __builtin_bswap64(load_le(p + 7 * (int64_t)r, nb)) | (unsigned long long)(rem < 8 ? (rem > 0 ? rem : 0) : 8);
  } else if (d.kind == kFixed) {
    const int left = (int)len - 8 * r;
    k = __builtin_bswap64(load_le(p + 8 * r, left < 8 ? left : 8));
  } else {
    k = load_le(p + 8 * ((int)len / 8 - 1 - r), 8);
    if (r == 0) k ^= 1ull << 63;
  }
  return d.descending ? ~k : k;
}

// does a row whose round-r key is k take part in round r + 1?
__device__ __forceinline__ bool continues(const BinDesc& d, unsigned long long k, int r) {
  if (d.kind == kVar) return ((d.descending ? ~k : k) & 0xFFull) == 8;
  return r + 1 < d.nrounds;
}

// round 0 as pass (1) of sort_by_column: digit = category (rest 0, null 2; reversed for nulls at start)
struct BinColumn {
  BinDesc d;
  const unsigned* rows_in;
  int nulls_at_start;
  __device__ __forceinline__ void load(int64_t i, unsigned long long* key, unsigned* row, unsigned* digit) const {
    const unsigned r = rows_in ? rows_in[i] : (unsigned)i;
    const bool null = !ah_bit(d.valid, d.off + r);
    *key = null ? 0ull : bin_key(d, r, 0);
    *row = r;
    const unsigned cat = null ? 2u : 0u;
    *digit = nulls_at_start ? 2u - cat : cat;
  }
};

// LSD pass over the run index of the pairs' source entries: (key, entry), digit = a byte of run[entry]
struct RunPairs {
  const unsigned long long* keys;
  const unsigned* idx;
  const unsigned* run;
  int shift;
  __device__ __forceinline__ void load(int64_t i, unsigned long long* key, unsigned* row, unsigned* digit) const {
    *key = keys[i];
    *row = idx[i];
    *digit = (run[*row] >> shift) & 255u;
  }
};

// ---- finding the rows still tied ----------------------------------------------------------------
// entries j of a round: key keys[j], position pos[j] in b.ra (pos == nullptr: base + j), run start flag head[j] (nullptr:
// only entry 0).  tied(j): entries j − 1 and j are in the same run, have equal keys and continue.
struct Ties {
  BinDesc d;
  int r;
  const unsigned long long* keys;
  const unsigned* pos;
  const unsigned* head;
  unsigned base;
  int64_t m;
  __device__ __forceinline__ bool tied(int64_t j) const {
    if (j <= 0 || j >= m) return false;
    if (head && head[j]) return false;
    const unsigned long long k = keys[j];
    return k == keys[j - 1] && continues(d, k, r);
  }
};

__global__ __launch_bounds__(kBlock) void tie_flags_kernel(Ties t, unsigned* __restrict__ flags) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < t.m; j += stride) flags[j] = (t.tied(j) || t.tied(j + 1)) ? 1u : 0u;
}

// scan = inclusive scan of the flags: the tied entries move to the front, in order, with a flag where a new run starts
__global__ __launch_bounds__(kBlock) void tie_compact_kernel(Ties t, const unsigned* __restrict__ scan, unsigned* __restrict__ pos_out,
                                                              unsigned* __restrict__ head_out) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < t.m; j += stride) {
    const bool prev = t.tied(j);
    if (!(prev || t.tied(j + 1))) continue;
    const unsigned k = scan[j] - 1;
    pos_out[k] = t.pos ? t.pos[j] : t.base + (unsigned)j;
    head_out[k] = prev ? 0u : 1u;
  }
}

// scan = inclusive scan of head: run[j] = run index, run_start[s] = first entry of run s, run_start[nruns] = m
__global__ __launch_bounds__(kBlock) void run_index_kernel(const unsigned* __restrict__ scan, const unsigned* __restrict__ head, int64_t m,
                                                            unsigned* __restrict__ run, unsigned* __restrict__ run_start) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += stride) {
    const unsigned s = scan[j] - 1;
    run[j] = s;
    if (head[j]) run_start[s] = (unsigned)j;
    if (j == m - 1) run_start[s + 1] = (unsigned)m;
  }
}

__global__ __launch_bounds__(kBlock) void longest_run_kernel(const unsigned* __restrict__ run_start, int64_t nruns, unsigned* __restrict__ out) {
  unsigned mx = 0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x; s < nruns; s += stride) {
    const unsigned len = run_start[s + 1] - run_start[s];
    mx = len > mx ? len : mx;
  }
  mx = ah_wave_max(mx);
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(out, mx);
}

// ---- a later round ---------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void round_keys_kernel(BinDesc d, int r, const unsigned* __restrict__ pos, int64_t m, const unsigned* __restrict__ ra,
                                                             unsigned long long* __restrict__ keys, unsigned* __restrict__ rows, unsigned* __restrict__ idx) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x; j < m; j += stride) {
    const unsigned row = ra[pos[j]];
    rows[j] = row;
    keys[j] = bin_key(d, row, r);
    idx[j] = (unsigned)j;
  }
}

// one wave per run of 2 … kWaveSeg entries: bitonic network over (key, position in the run) — stable because positions are
// distinct and in the current order — then the rows go back to the run's positions in b.ra, the keys to their entries
__global__ __launch_bounds__(64) void run_bitonic_kernel(const unsigned* __restrict__ run_start, const unsigned* __restrict__ pos,
                                                          const unsigned* __restrict__ rows, unsigned long long* __restrict__ keys,
                                                          unsigned* __restrict__ ra) {
  __shared__ unsigned long long s_k[kWaveSeg];
  __shared__ unsigned short s_t[kWaveSeg];
  const unsigned j0 = run_start[blockIdx.x], len = run_start[blockIdx.x + 1] - j0;
  const unsigned lane = threadIdx.x;
  unsigned P = 2;
  while (P < len) P <<= 1;
  for (unsigned t = lane; t < P; t += 64) {
    s_k[t] = t < len ? keys[j0 + t] : ~0ull;  // padding sorts last: its tags are above every real one
    s_t[t] = (unsigned short)t;
  }
  __syncthreads();
  for (unsigned k = 2; k <= P; k <<= 1) {
    for (unsigned h = k >> 1; h > 0; h >>= 1) {
      for (unsigned t = lane; t < P / 2; t += 64) {
        const unsigned i = (t / h) * 2 * h + (t % h), l = i + h;
        const unsigned long long ki = s_k[i], kl = s_k[l];
        const unsigned short ti = s_t[i], tl = s_t[l];
        const bool gt = ki > kl || (ki == kl && ti > tl);
        if (gt == ((i & k) == 0)) { s_k[i] = kl; s_k[l] = ki; s_t[i] = tl; s_t[l] = ti; }
      }
      __syncthreads();
    }
  }
  for (unsigned t = lane; t < len; t += 64) {
    ra[pos[j0 + t]] = rows[j0 + s_t[t]];
    keys[j0 + t] = s_k[t];
  }
}

__global__ __launch_bounds__(kBlock) void write_back_kernel(const unsigned* __restrict__ idx, int64_t m, const unsigned* __restrict__ pos,
                                                             const unsigned* __restrict__ rows, unsigned* __restrict__ ra) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < m; i += stride) ra[pos[i]] = rows[idx[i]];
}

// which key bytes vary over keys[0, m)
int varying_bytes(ah_ctx* c, SortBuffers& b, const unsigned long long* keys, int64_t m, unsigned long long* varying) {
  const unsigned agrid = std::min(ah_stream_grid(c, ah_ceil_div(m, kBlock), 4), (unsigned)kAndOrGrid);
  and_or_kernel<<<agrid, kBlock, 0, c->stream>>>(keys, m, b.andor);
  AH_LAUNCH_CHECK(c);
  std::vector<unsigned long long> parts((size_t)agrid * 4);
  AH_HIP(c, hipMemcpyAsync(parts.data(), b.andor, parts.size() * 8, hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipStreamSynchronize(c->stream));
  unsigned long long a = ~0ull, o = 0ull;
  for (unsigned g = 0; g < agrid; g++) { a &= parts[g * 4]; o |= parts[g * 4 + 1]; }
  *varying = a ^ o;
  return AH_OK;
}

}  // namespace

bool ah_sort_is_binary(int type) {
  return type == AH_BINARY || type == AH_LARGE_BINARY || type == AH_FIXED_SIZE_BINARY || type == AH_DECIMAL128 || type == AH_DECIMAL256;
}

int ah_sort_by_binary(ah_ctx* c, SortBuffers& b, const SortCol& col, int64_t n, const unsigned* rows_in) {
  BinDesc d;
  d.kind = col.type == AH_BINARY || col.type == AH_LARGE_BINARY ? kVar : col.type == AH_FIXED_SIZE_BINARY ? kFixed : kDecimal;
  d.ow = col.type == AH_BINARY ? 4 : col.type == AH_LARGE_BINARY ? 8 : 0;
  d.nrounds = d.kind == kFixed ? (col.width + 7) / 8 : d.kind == kDecimal ? col.width / 8 : 0;
  d.descending = col.descending;
  d.rows = byte_rows(d.ow, col.offsets, col.data, col.width, col.off);
  d.valid = col.valid;
  d.off = col.off;
  const int64_t ntiles = ah_ceil_div(n, (int64_t)kTile * tiles_per_block(n));
  int rc;
  // round 0 over all rows: partition off the nulls, then the LSD passes over the varying key bytes
  BinColumn src{d, rows_in, col.nulls_at_start};
  if ((rc = radix_pass(c, src, n, b.hist, b.offs, b.ka, b.ra)) != AH_OK) return rc;
  unsigned ends[3];
  for (int k = 0; k < 3; k++)
    AH_HIP(c, hipMemcpyAsync(&c->pinned[k], b.offs + ((int64_t)k + 1) * ntiles - 1, 4, hipMemcpyDeviceToHost, c->stream));
  AH_HIP(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 3; k++) ends[k] = *(volatile unsigned*)&c->pinned[k];
  const int64_t rest_lo = col.nulls_at_start ? ends[1] : 0;
  const int64_t rest_n = col.nulls_at_start ? (int64_t)ends[2] - ends[1] : ends[0];
  if (rest_n <= 1) return AH_OK;
  unsigned long long *kcur = b.ka + rest_lo, *kalt = b.kb + rest_lo;
  unsigned *rcur = b.ra + rest_lo, *ralt = b.rb + rest_lo;
  unsigned long long varying;
  if ((rc = varying_bytes(c, b, kcur, rest_n, &varying)) != AH_OK) return rc;
  for (int by = 0; by < 8; by++) {
    if (((varying >> (8 * by)) & 0xFFull) == 0) continue;
    Pairs p{kcur, rcur, 8 * by};
    if ((rc = radix_pass(c, p, rest_n, b.hist, b.offs, kalt, ralt)) != AH_OK) return rc;
    std::swap(kcur, kalt);
    std::swap(rcur, ralt);
  }
  if (rcur != b.ra + rest_lo) AH_HIP(c, hipMemcpyAsync(b.ra + rest_lo, rcur, (size_t)rest_n * 4, hipMemcpyDeviceToDevice, c->stream));
  // later rounds over the rows still tied
  unsigned *pos = b.bin[0], *pos2 = b.bin[1], *head = b.bin[2], *head2 = b.bin[3], *scan = b.bin[4], *rows = b.bin[5], *run = b.bin[6],
           *run_start = b.bin[7];
  const unsigned long long* keys = kcur;
  int64_t m = rest_n;
  for (int r = 0;; r++) {
    if (d.kind != kVar && r + 1 >= d.nrounds) break;  // the last chunk of a fixed width: ties are final
    Ties t{d, r, keys, r == 0 ? nullptr : pos, r == 0 ? nullptr : head, (unsigned)rest_lo, m};
    const unsigned grid = ah_stream_grid(c, ah_ceil_div(m, kBlock), 8);
    tie_flags_kernel<<<grid, kBlock, 0, c->stream>>>(t, run);
    AH_LAUNCH_CHECK(c);
    if ((rc = ah_cumulative_sum(c, AH_UINT32, run, nullptr, 0, m, nullptr, 0, 0, scan, nullptr, nullptr)) != AH_OK) return rc;
    tie_compact_kernel<<<grid, kBlock, 0, c->stream>>>(t, scan, pos2, head2);
    AH_LAUNCH_CHECK(c);
    AH_HIP(c, hipMemcpyAsync(&c->pinned[0], scan + m - 1, 4, hipMemcpyDeviceToHost, c->stream));
    AH_HIP(c, hipStreamSynchronize(c->stream));
    const int64_t m2 = *(volatile unsigned*)&c->pinned[0];
    if (m2 == 0) break;
    std::swap(pos, pos2);
    std::swap(head, head2);
    m = m2;
    // the runs: index of every entry, first entry of every run, the longest run
    const unsigned g2 = ah_stream_grid(c, ah_ceil_div(m, kBlock), 8);
    if ((rc = ah_cumulative_sum(c, AH_UINT32, head, nullptr, 0, m, nullptr, 0, 0, scan, nullptr, nullptr)) != AH_OK) return rc;
    run_index_kernel<<<g2, kBlock, 0, c->stream>>>(scan, head, m, run, run_start);
    AH_LAUNCH_CHECK(c);
    AH_HIP(c, hipMemcpyAsync(&c->pinned[0], scan + m - 1, 4, hipMemcpyDeviceToHost, c->stream));
    AH_HIP(c, hipStreamSynchronize(c->stream));
    const int64_t nruns = *(volatile unsigned*)&c->pinned[0];
    unsigned* longest = (unsigned*)b.andor;
    AH_HIP(c, hipMemsetAsync(longest, 0, 4, c->stream));
    longest_run_kernel<<<ah_stream_grid(c, ah_ceil_div(nruns, kBlock), 8), kBlock, 0, c->stream>>>(run_start, nruns, longest);
    AH_LAUNCH_CHECK(c);
    AH_HIP(c, hipMemcpyAsync(&c->pinned[1], longest, 4, hipMemcpyDeviceToHost, c->stream));
    AH_HIP(c, hipStreamSynchronize(c->stream));
    const unsigned maxlen = *(volatile unsigned*)&c->pinned[1];
    // round r + 1: keys of the tied rows, sorted inside their runs
    round_keys_kernel<<<g2, kBlock, 0, c->stream>>>(d, r + 1, pos, m, b.ra, b.ka, rows, b.rb);
    AH_LAUNCH_CHECK(c);
    keys = b.ka;
    if (maxlen <= (unsigned)kWaveSeg) {
      run_bitonic_kernel<<<(unsigned)nruns, 64, 0, c->stream>>>(run_start, pos, rows, b.ka, b.ra);
      AH_LAUNCH_CHECK(c);
      continue;
    }
    // a run too long for one wave: all tied rows by stable LSD passes over (run index, key), key bytes first
    if ((rc = varying_bytes(c, b, b.ka, m, &varying)) != AH_OK) return rc;
    unsigned long long *k1 = b.ka, *k2 = b.kb;
    unsigned *i1 = b.rb, *i2 = scan;
    bool moved = false;
    for (int by = 0; by < 8; by++) {
      if (((varying >> (8 * by)) & 0xFFull) == 0) continue;
      Pairs p{k1, i1, 8 * by};
      if ((rc = radix_pass(c, p, m, b.hist, b.offs, k2, i2)) != AH_OK) return rc;
      std::swap(k1, k2);
      std::swap(i1, i2);
      moved = true;
    }
    for (int by = 0; by < 4 && ((unsigned long long)(nruns - 1) >> (8 * by)) != 0; by++) {
      RunPairs p{k1, i1, run, 8 * by};
      if ((rc = radix_pass(c, p, m, b.hist, b.offs, k2, i2)) != AH_OK) return rc;
      std::swap(k1, k2);
      std::swap(i1, i2);
      moved = true;
    }
    keys = k1;
    if (moved) {
      write_back_kernel<<<g2, kBlock, 0, c->stream>>>(i1, m, pos, rows, b.ra);
      AH_LAUNCH_CHECK(c);
    }
  }
  return AH_OK;
}
