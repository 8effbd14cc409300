// ah_string_transform.hip (include/arrowhip_strings.h) — the string transforms whose result
// is one contiguous sub-range of the row's bytes: utf8_slice_codeunits, binary_slice, ascii_trim*, utf8_trim*, and — the whole row
// through a byte map — ascii_upper / ascii_lower (no reference analogue; Arrow C++'s semantics).
//
// One pair of kernels serves all of them, split like ah_take_binary_offsets / ah_take_binary_data (ah_varlen.hip):
//   ah_string_ranges  a row per lane: the row's offsets, its validity bit, and as many of its bytes as the op has to look at — none
//                     for binary_slice and the whole row, the trimmed bytes plus one for a trim, |start| and |stop| code points from
//                     the end they count from for a slice.  A lane walks kLaneWalk bytes alone; a row that needs more is handed to
//                     the whole wave, one pending row after another, 64 bytes per step (a ballot of "not a continuation byte" /
//                     "not in the set" per step).  The byte set of ascii_*trim is a 256-bit table, the code-point set of utf8_*trim
//                     a sorted array of the code points' bytes packed into 32-bit keys; both sit in LDS.  The kernel writes the
//                     source start and the length of every row; the lengths go through the scan of ah_scan.hip (ah_cumulative_sum)
//                     into the output offsets, and the total comes home — the call's one synchronisation.
//   ah_string_gather  work goes by OUTPUT bytes: [0, total) is cut into tiles of T bytes (context option string_tile_bytes), a fixed
//                     grid takes contiguous runs of tiles, a workgroup binary-searches the output offsets once for the first row of
//                     its run and walks forward, a row per thread, every row clipped to the run.  What is left of a row is copied by
//                     its lane alone (≤ kLaneCopy bytes), by the wave (≤ kWaveCopy, 256 bytes per step) or by the whole workgroup
//                     (4 KiB per step, 16 bytes per thread) — so a row that covers many runs is copied by all of them, and every
//                     output byte has exactly one writer.  The optional byte map sits in LDS.
#include "ah_bytes.h"
#include "ah_strings.h"
#include "ah_varout.h"
#include "../../include/arrowhip_strings.h"

namespace {

constexpr int kLaneWalk = 64;      // bytes of a row a lane looks at alone (ranges)
constexpr int kLaneCopy = 64;      // bytes of a clipped row a lane copies alone (gather)
constexpr int kWaveCopy = 4096;    // … the wave copies; longer: the workgroup
constexpr int kMaxKeys = AH_STX_MAX_CHARS;   // code points of a set: at most one per byte

struct RangeOp {
  int op, has_stop, sides, nkeys;
  long long start, stop;
};

// WAVE: all 64 lanes hold the same row and look at 64 consecutive bytes per step; else one lane walks alone, a byte per step, and
// gives up (→ −1 / false) when its budget of kLaneWalk bytes is spent.
template <bool WAVE>
__device__ __forceinline__ unsigned long long cmask(bool p) {
  if constexpr (WAVE) return __ballot(p);
  else return p ? 1ull : 0ull;
}
template <bool WAVE>
__device__ __forceinline__ bool spend(int* budget) {
  if constexpr (WAVE) return true;
  else return --*budget >= 0;
}

// where code point k (0-based) of the row starts, len if it has fewer; −1: out of budget
template <bool WAVE>
__device__ __forceinline__ long long nth_start_fwd(const uint8_t* p, long long len, long long k, int* budget) {
  constexpr int W = WAVE ? 64 : 1;
  const int li = WAVE ? ah_lane() : 0;
  if (k >= len) return len;   // (a code point has at least one byte)
  for (long long x0 = 0; x0 < len; x0 += W) {
    if (!spend<WAVE>(budget)) return -1;
    const long long x = x0 + li;
    const bool f = x < len && (x == 0 || !is_cont(p[x]));
    const unsigned long long m = cmask<WAVE>(f);
    const int cnt = __popcll(m);
    if (k < cnt) {
      if constexpr (!WAVE) return x0;
      else {
        const unsigned long long below = m & ((1ull << li) - 1);
        const unsigned long long hit = __ballot(f && __popcll(below) == (int)k);
        return x0 + __ffsll((long long)hit) - 1;
      }
    }
    k -= cnt;
  }
  return len;
}
// where the k-th code point from the row's end (k ≥ 1) starts, 0 if it has fewer; −1: out of budget
template <bool WAVE>
__device__ __forceinline__ long long nth_start_rev(const uint8_t* p, long long len, long long k, int* budget) {
  constexpr int W = WAVE ? 64 : 1;
  const int li = WAVE ? ah_lane() : 0;
  if (k >= len) return 0;
  for (long long hi = len; hi > 0; hi -= W) {
    if (!spend<WAVE>(budget)) return -1;
    const long long x = hi - 1 - li;   // lane 0 looks at the last byte
    const bool f = x >= 0 && (x == 0 || !is_cont(p[x]));
    const unsigned long long m = cmask<WAVE>(f);
    const int cnt = __popcll(m);
    if (k <= cnt) {
      if constexpr (!WAVE) return x;
      else {
        const unsigned long long below = m & ((1ull << li) - 1);
        const unsigned long long hit = __ballot(f && __popcll(below) == (int)(k - 1));
        return hi - 1 - (__ffsll((long long)hit) - 1);
      }
    }
    k -= cnt;
  }
  return 0;
}

__device__ __forceinline__ bool in_byte_set(const unsigned* set, uint8_t b) { return (set[b >> 5] >> (b & 31)) & 1u; }

// the code point that starts at byte x of the row (len bytes): are its bytes in the sorted key array?  More than 4 bytes: never.
__device__ __forceinline__ bool in_key_set(const uint8_t* p, long long x, long long len, const unsigned* keys, int nkeys) {
  unsigned key = p[x];
  int j = 1;
  while (x + j < len && is_cont(p[x + j])) {
    if (j >= 4) return false;
    key |= (unsigned)p[x + j] << (8 * j);
    j++;
  }
  int lo = 0, hi = nkeys;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo < nkeys && keys[lo] == key;
}

// The trims over bytes [a, b) of the row; CP: code points of the key array, else bytes of the 256-bit table.  a is where a code point
// starts, b where one ends.  → the new a (left) / the new b (right); −1: out of budget.
template <bool WAVE, bool CP>
__device__ __forceinline__ long long trim_left(const uint8_t* p, long long len, long long a, long long b, const unsigned* set, int nkeys, int* budget) {
  constexpr int W = WAVE ? 64 : 1;
  const int li = WAVE ? ah_lane() : 0;
  for (long long x0 = a; x0 < b; x0 += W) {
    if (!spend<WAVE>(budget)) return -1;
    const long long x = x0 + li;
    bool stop = x >= b;
    if (!stop) {
      if constexpr (CP) {
        if (x == a || !is_cont(p[x])) stop = !in_key_set(p, x, len, set, nkeys);   // (a continuation byte goes with the code point in front of it)
      } else {
        stop = !in_byte_set(set, p[x]);
      }
    }
    const unsigned long long m = cmask<WAVE>(stop);
    if (m) {
      const long long at = x0 + __ffsll((long long)m) - 1;
      return at < b ? at : b;
    }
  }
  return b;
}
template <bool WAVE, bool CP>
__device__ __forceinline__ long long trim_right(const uint8_t* p, long long len, long long a, long long b, const unsigned* set, int nkeys, int* budget) {
  constexpr int W = WAVE ? 64 : 1;
  const int li = WAVE ? ah_lane() : 0;
  long long e = b;   // everything from e on is trimmed; a code point ends at e
  for (long long hi = b; hi > a; hi -= W) {
    if (!spend<WAVE>(budget)) return -1;
    const long long x = hi - 1 - li;   // lane 0 looks at the last byte
    if constexpr (CP) {
      const bool flag = x >= a && (x == a || !is_cont(p[x]));
      const bool fail = flag && !in_key_set(p, x, len, set, nkeys);
      const unsigned long long mflag = cmask<WAVE>(flag), mfail = cmask<WAVE>(fail);
      if (mfail) {   // the last code point that stays: it ends where the next one of this step starts, or at e
        const int l = __ffsll((long long)mfail) - 1;
        const unsigned long long above = mflag & ((1ull << l) - 1);
        return above ? hi - 1 - (63 - __clzll((long long)above)) : e;
      }
      if (mflag) e = hi - 1 - (63 - __clzll((long long)mflag));   // all of them go: up to the first start of this step
    } else {
      const bool stop = x < a || !in_byte_set(set, p[x]);
      const unsigned long long m = cmask<WAVE>(stop);
      if (m) {
        const long long at = hi - (__ffsll((long long)m) - 1);
        return at > a ? at : a;
      }
    }
  }
  return CP ? e : a;
}

// the range [*a, *b) of the row's bytes the op keeps; false: out of budget (the lane's answer is the wave's to give)
template <int OP, bool WAVE>
__device__ __forceinline__ bool row_range(const RangeOp& o, const uint8_t* p, long long len, const unsigned* set, long long* a, long long* b) {
  int budget = kLaneWalk;
  long long x = 0, y = len;
  switch (OP) {   // (the op is the kernel's template parameter: one walk per instantiation)
    case AH_STX_SLICE_BYTES: {
      x = o.start < 0 ? (o.start + len < 0 ? 0 : o.start + len) : (o.start > len ? len : o.start);
      if (o.has_stop) y = o.stop < 0 ? (o.stop + len < 0 ? 0 : o.stop + len) : (o.stop > len ? len : o.stop);
      break;
    }
    case AH_STX_SLICE_CODEPOINTS: {
      if (o.has_stop && (o.start < 0) == (o.stop < 0) && o.stop <= o.start) {   // empty whatever the row holds
        x = y = 0;
        break;
      }
      x = o.start >= 0 ? nth_start_fwd<WAVE>(p, len, o.start, &budget) : nth_start_rev<WAVE>(p, len, o.start <= -len ? len : -o.start, &budget);
      if (x < 0) return false;
      if (o.has_stop) {
        y = o.stop >= 0 ? nth_start_fwd<WAVE>(p, len, o.stop, &budget) : nth_start_rev<WAVE>(p, len, o.stop <= -len ? len : -o.stop, &budget);
        if (y < 0) return false;
      }
      break;
    }
    case AH_STX_TRIM_BYTES: {
      if (o.sides & AH_STX_LEFT) x = trim_left<WAVE, false>(p, len, 0, len, set, 0, &budget);
      if (x < 0) return false;
      if (o.sides & AH_STX_RIGHT) y = trim_right<WAVE, false>(p, len, x, len, set, 0, &budget);
      if (y < 0) return false;
      break;
    }
    case AH_STX_TRIM_CODEPOINTS: {
      if (o.sides & AH_STX_LEFT) x = trim_left<WAVE, true>(p, len, 0, len, set, o.nkeys, &budget);
      if (x < 0) return false;
      if (o.sides & AH_STX_RIGHT) y = trim_right<WAVE, true>(p, len, x, len, set, o.nkeys, &budget);
      if (y < 0) return false;
      break;
    }
    default: break;   // AH_STX_WHOLE
  }
  if (y < x) y = x;
  *a = x;
  *b = y;
  return true;
}

template <typename OffT, int OP>
__global__ __launch_bounds__(kBlock) void ranges_kernel(const OffT* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                        const uint8_t* __restrict__ valid, int64_t voff, int64_t n, RangeOp o,
                                                        const unsigned* __restrict__ set_words, int nset, OffT* __restrict__ starts,
                                                        long long* __restrict__ lens) {
  __shared__ unsigned s_set[kMaxKeys];
  for (int j = threadIdx.x; j < nset; j += kBlock) s_set[j] = set_words[j];
  __syncthreads();
  const int lane = ah_lane();
  const int64_t nchunks = (n + 63) >> 6;
  const int64_t wave_stride = (int64_t)gridDim.x * (kBlock / 64);
  for (int64_t ch = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); ch < nchunks; ch += wave_stride) {
    const int64_t i = ch * 64 + lane;
    const unsigned long long vbits = ah_wave_bits64(valid, voff + ch * 64, n - ch * 64);
    long long rs = 0, len = 0, a = 0, b = 0;
    const uint8_t* p = nullptr;
    bool pend = false;
    if (i < n) {
      rs = (long long)offsets[i];
      if ((vbits >> lane) & 1ull) {
        len = (long long)offsets[i + 1] - rs;
        p = data + rs;
        pend = !row_range<OP, false>(o, p, len, s_set, &a, &b);
      }
    }
    for_pending_lanes(__ballot(pend), [&](int l) {   // the rows a lane could not finish alone: the whole wave, one after another
      const uint8_t* wp = (const uint8_t*)(uintptr_t)__shfl((long long)(uintptr_t)p, l);
      const long long wl = __shfl(len, l);
      long long wa = 0, wb = 0;
      row_range<OP, true>(o, wp, wl, s_set, &wa, &wb);
      if (lane == l) {
        a = wa;
        b = wb;
      }
    });
    if (i < n) {
      starts[i] = (OffT)(rs + a);
      lens[i] = b - a;
    }
  }
}

// ---- gather ------------------------------------------------------------------------------------------------------------------------------
struct BigRow { const uint8_t* src; uint8_t* dst; long long len; };
struct ByteMap { uint8_t b[256]; };

template <bool MAP>
__device__ __forceinline__ unsigned map4(unsigned w, const uint8_t* m) {
  if constexpr (!MAP) return w;
  else return (unsigned)m[w & 255] | ((unsigned)m[(w >> 8) & 255] << 8) | ((unsigned)m[(w >> 16) & 255] << 16) | ((unsigned)m[w >> 24] << 24);
}
template <bool MAP>
__device__ __forceinline__ uint8_t map1(uint8_t b, const uint8_t* m) { return MAP ? m[b] : b; }

template <typename OffT, bool MAP>
__global__ __launch_bounds__(kBlock) void gather_kernel(const uint8_t* __restrict__ data, const OffT* __restrict__ starts,
                                                        const OffT* __restrict__ oo, int64_t n, const ByteMap map, int T,
                                                        uint8_t* __restrict__ out) {
  __shared__ long long s_first;
  __shared__ int s_nbig;
  __shared__ uint8_t s_map[256];
  __shared__ BigRow s_big[kBlock];
  const int64_t total = (int64_t)oo[n];
  int64_t t0, t1;   // the first row of the run: the first that ends behind its first byte (that byte is in front of total = oo[n]: row n − 1 is one)
  if (!tile_run((total + T - 1) / T, T, n - 1, [&](int64_t i, int64_t x) { return (int64_t)oo[i + 1] <= x; }, &t0, &t1, &s_first)) return;
  const int64_t lo = t0 * T, hi = t1 * T < total ? t1 * T : total;   // this workgroup's output bytes
  if (threadIdx.x == 0) s_nbig = 0;
  if (MAP) s_map[threadIdx.x] = map.b[threadIdx.x];   // (kBlock = 256; the map travels as a kernel argument: nothing to upload)
  __syncthreads();
  const int lane = ah_lane();
  for (int64_t it = s_first;; it += kBlock) {
    const int64_t i = it + threadIdx.x;
    bool in = false;
    const uint8_t* src = nullptr;
    uint8_t* dst = nullptr;
    long long len = 0;
    if (i < n) {
      const int64_t o0 = (int64_t)oo[i];
      in = o0 < hi;
      if (in) {
        const int64_t o1 = (int64_t)oo[i + 1];
        const int64_t d0 = o0 > lo ? o0 : lo, d1 = o1 < hi ? o1 : hi;   // the row clipped to [lo, hi)
        len = d1 - d0;
        if (len > 0) {
          src = data + (int64_t)starts[i] + (d0 - o0);
          dst = out + d0;
        }
      }
    }
    if (len > kWaveCopy) {
      s_big[atomicAdd(&s_nbig, 1)] = BigRow{src, dst, len};
    } else if (len > 0 && len <= kLaneCopy) {
      long long b = 0;
      for (; b + 4 <= len; b += 4) ((U32u*)(dst + b))->v = map4<MAP>(((const U32u*)(src + b))->v, s_map);
      for (; b < len; b++) dst[b] = map1<MAP>(src[b], s_map);
    }
    for_pending_lanes(__ballot(len > kLaneCopy && len <= kWaveCopy), [&](int l) {   // the wave's rows, one after another: 4 bytes per lane and step
      const uint8_t* ws = (const uint8_t*)(uintptr_t)__shfl((long long)(uintptr_t)src, l);
      uint8_t* wd = (uint8_t*)(uintptr_t)__shfl((long long)(uintptr_t)dst, l);
      const long long wl = __shfl(len, l);
      for (long long b = (long long)lane * 4; b + 4 <= wl; b += 256) ((U32u*)(wd + b))->v = map4<MAP>(((const U32u*)(ws + b))->v, s_map);
      const long long tail = wl & ~3ll;
      if (lane < (int)(wl - tail)) wd[tail + lane] = map1<MAP>(ws[tail + lane], s_map);
    });
    const int cnt = __syncthreads_count(in);
    // How many rows were queued comes from a reduction over the threads' own `len`, never from a read of s_nbig: a wave that is
    // already in the next iteration may be adding to that counter.  s_nbig only hands out the slots; it is reset inside the
    // branch below, which every thread of the workgroup takes or none does.  (The barrier also makes the queued rows visible.)
    const int nbig = __syncthreads_count(len > kWaveCopy);
    if (nbig) {   // the workgroup's rows: 16 bytes per thread and step
      for (int k = 0; k < nbig; k++) {
        const BigRow r = s_big[k];
        const long long nvec = r.len >> 4;
        for (long long v = threadIdx.x; v < nvec; v += kBlock) {
          ah_vec16<uint8_t> x = ah_ld16<uint8_t>(r.src + v * 16);
          if (MAP) {
#pragma unroll
            for (int j = 0; j < 16; j++) x.v[j] = s_map[x.v[j]];
          }
          ah_st16<uint8_t>(r.dst + v * 16, x);
        }
        const long long tail = nvec << 4;
        if ((long long)threadIdx.x < r.len - tail) r.dst[tail + threadIdx.x] = map1<MAP>(r.src[tail + threadIdx.x], s_map);
      }
      __syncthreads();
      if (threadIdx.x == 0) s_nbig = 0;
      __syncthreads();
    }
    if (cnt < kBlock) break;
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
bool bad_buffer(const void* p, int width) { return !p || ((uintptr_t)p & (uintptr_t)(width - 1)); }

// `chars` as the sorted keys of its code points (their bytes, first byte lowest); false: not valid UTF-8
bool code_point_keys(const uint8_t* s, int64_t m, unsigned* keys, int* nkeys) {
  int k = 0;
  for (int64_t i = 0; i < m;) {
    const uint8_t b = s[i];
    const int len = b < 0x80 ? 1 : (b & 0xE0) == 0xC0 ? 2 : (b & 0xF0) == 0xE0 ? 3 : (b & 0xF8) == 0xF0 ? 4 : 0;
    if (!len || i + len > m) return false;
    unsigned cp = len == 1 ? b : b & (0xFF >> (len + 1)), key = b;
    for (int j = 1; j < len; j++) {
      if ((s[i + j] & 0xC0) != 0x80) return false;
      cp = (cp << 6) | (s[i + j] & 0x3F);
      key |= (unsigned)s[i + j] << (8 * j);
    }
    static const unsigned least[5] = {0, 0, 0x80, 0x800, 0x10000};
    if (cp < least[len] || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return false;   // overlong, out of range, a surrogate
    keys[k++] = key;
    i += len;
  }
  for (int i = 1; i < k; i++) {   // (at most 1024 keys: an insertion sort will do)
    const unsigned v = keys[i];
    int j = i;
    for (; j > 0 && keys[j - 1] > v; j--) keys[j] = keys[j - 1];
    keys[j] = v;
  }
  int u = 0;
  for (int i = 0; i < k; i++)
    if (i == 0 || keys[i] != keys[i - 1]) keys[u++] = keys[i];
  *nkeys = u;
  return true;
}

}  // namespace

AH_EXPORT int ah_string_ranges(ah_ctx* c, int op, int64_t start, int64_t stop, int has_stop, int sides, const uint8_t* chars, int64_t chars_len,
                               const ah_cmp_operand* operand, const uint8_t* valid, int64_t valid_offset, int64_t n, void* out_starts,
                               void* out_offsets, int64_t* out_total_bytes_host) {
  AH_ENTER(c);
  if (out_total_bytes_host) *out_total_bytes_host = 0;
  if (op < AH_STX_WHOLE || op > AH_STX_TRIM_CODEPOINTS) return ah_fail(c, AH_EINVALID, "string_ranges: bad op %d", op);
  if (int rc = check_column(c, "string_ranges", operand, n, false)) return rc;
  if (valid_offset < 0) return ah_fail(c, AH_EINVALID, "string_ranges: negative validity offset");
  const bool trim = op == AH_STX_TRIM_BYTES || op == AH_STX_TRIM_CODEPOINTS;
  unsigned set_words[kMaxKeys];
  int nset = 0;
  RangeOp o{op, has_stop ? 1 : 0, sides, 0, (long long)start, (long long)stop};
  if (trim) {
    if (sides < AH_STX_LEFT || sides > (AH_STX_LEFT | AH_STX_RIGHT)) return ah_fail(c, AH_EINVALID, "string_ranges: bad sides %d", sides);
    if (chars_len < 0 || chars_len > AH_STX_MAX_CHARS) return ah_fail(c, AH_EINVALID, "string_ranges: %lld characters' bytes outside 0 … %d", (long long)chars_len, AH_STX_MAX_CHARS);
    if (chars_len > 0 && !chars) return ah_fail(c, AH_EINVALID, "string_ranges: null characters");
    if (op == AH_STX_TRIM_BYTES) {
      nset = 8;
      memset(set_words, 0, 8 * sizeof(unsigned));
      for (int64_t j = 0; j < chars_len; j++) set_words[chars[j] >> 5] |= 1u << (chars[j] & 31);
    } else {
      if (!code_point_keys(chars, chars_len, set_words, &nset)) return ah_fail(c, AH_EINVALID, "string_ranges: the characters are not valid UTF-8");
      o.nkeys = nset;
    }
  }
  const int ow = operand->offset_width;
  if (n > 0 && (bad_buffer(out_starts, ow) || bad_buffer(out_offsets, ow))) return ah_fail(c, AH_EINVALID, "string_ranges: null or misaligned output");
  if (n == 0) return AH_OK;
  // the rows' lengths and their scan, the set in front of them; a row's result is never longer than the row: no overflow to look for
  VarOut v;
  if (int rc = varout_begin(c, n, sizeof(set_words), /*can_overflow=*/false, &v)) return rc;
  unsigned* set_dev = (unsigned*)v.extra;
  // (set_words is this function's stack: the copy is read by the time the call returns — it ends in a synchronisation, also where it fails)
  if (nset > 0) AH_HIP(c, hipMemcpyAsync(set_dev, set_words, (size_t)nset * sizeof(unsigned), hipMemcpyHostToDevice, c->stream));
  const ByteRows rows = byte_rows(ow, operand->offsets, operand->data, 0, operand->off);
  const unsigned grid = chunk_grid(c, n);
  auto launch = [&](auto tag) {
    constexpr int OP = decltype(tag)::value;
    if (ow == 4) ranges_kernel<int32_t, OP><<<grid, kBlock, 0, c->stream>>>((const int32_t*)rows.offsets, rows.data, valid, valid_offset, n, o, set_dev, nset, (int32_t*)out_starts, v.lens);
    else ranges_kernel<long long, OP><<<grid, kBlock, 0, c->stream>>>((const long long*)rows.offsets, rows.data, valid, valid_offset, n, o, set_dev, nset, (long long*)out_starts, v.lens);
  };
  switch (op) {
    case AH_STX_SLICE_BYTES: launch(std::integral_constant<int, AH_STX_SLICE_BYTES>{}); break;
    case AH_STX_SLICE_CODEPOINTS: launch(std::integral_constant<int, AH_STX_SLICE_CODEPOINTS>{}); break;
    case AH_STX_TRIM_BYTES: launch(std::integral_constant<int, AH_STX_TRIM_BYTES>{}); break;
    case AH_STX_TRIM_CODEPOINTS: launch(std::integral_constant<int, AH_STX_TRIM_CODEPOINTS>{}); break;
    default: launch(std::integral_constant<int, AH_STX_WHOLE>{}); break;
  }
  if (hipGetLastError() != hipSuccess) {
    (void)hipStreamSynchronize(c->stream);
    return ah_fail(c, AH_EHIP, "string_ranges: the launch failed");
  }
  int rc = varout_enqueue(c, v, n, ow, out_offsets, /*caller_words=*/false);
  int64_t total = 0;
  bool overflow = false;
  if (rc == AH_OK) rc = varout_finish(c, v, &total, &overflow);
  if (rc != AH_OK) {
    (void)hipStreamSynchronize(c->stream);   // (the failed step left its own message)
    return rc;
  }
  if (out_total_bytes_host) *out_total_bytes_host = total;
  return AH_OK;
}

AH_EXPORT int ah_string_gather(ah_ctx* c, const ah_cmp_operand* operand, const void* starts, const void* out_offsets, int64_t n,
                               const uint8_t* map, uint8_t* out_data) {
  AH_ENTER(c);
  if (int rc = check_column(c, "string_gather", operand, n, false)) return rc;
  if (n == 0) return AH_OK;
  const int ow = operand->offset_width;
  if (bad_buffer(starts, ow) || bad_buffer(out_offsets, ow)) return ah_fail(c, AH_EINVALID, "string_gather: null or misaligned starts / offsets");
  if (!out_data) return ah_fail(c, AH_EINVALID, "string_gather: null output data");
  ByteMap map_dev;   // the map goes to the kernel by value, in its arguments: read here, nothing of the caller's is used after the call
  if (map) memcpy(map_dev.b, map, 256);
  else memset(map_dev.b, 0, 256);
  const int T = tile_bytes(c);
  const unsigned grid = tile_grid(c);
  if (ow == 4) {
    if (map) gather_kernel<int32_t, true><<<grid, kBlock, 0, c->stream>>>(operand->data, (const int32_t*)starts, (const int32_t*)out_offsets, n, map_dev, T, out_data);
    else gather_kernel<int32_t, false><<<grid, kBlock, 0, c->stream>>>(operand->data, (const int32_t*)starts, (const int32_t*)out_offsets, n, map_dev, T, out_data);
  } else {
    if (map) gather_kernel<long long, true><<<grid, kBlock, 0, c->stream>>>(operand->data, (const long long*)starts, (const long long*)out_offsets, n, map_dev, T, out_data);
    else gather_kernel<long long, false><<<grid, kBlock, 0, c->stream>>>(operand->data, (const long long*)starts, (const long long*)out_offsets, n, map_dev, T, out_data);
  }
  AH_LAUNCH_CHECK(c);
  return AH_OK;
}
