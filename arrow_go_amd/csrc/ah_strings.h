// ah_strings.h — what the two string files share (ah_string_match.hip: the predicates; ah_string_transform.hip: slice, trim, the case
// mappings): the tiles a byte range is cut into (context option string_tile_bytes) and the grids over them, a workgroup's run of
// tiles with the first row of that run, the column check, the UTF-8 continuation-byte test.
#pragma once
#include "ah_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kDefaultTile = 16384;   // bytes per tile: in ah_string_match.hip 16 KiB + bit array + pattern ≈ 19 KiB of LDS, eight workgroups per CU
constexpr int kMinTile = 64, kMaxTile = 32768;
constexpr int kWgPerCu = 8;

__device__ __forceinline__ bool is_cont(uint8_t b) { return (b & 0xC0) == 0x80; }   // 10xxxxxx: a UTF-8 continuation byte

// A byte range of `ntiles` tiles of T bytes, a contiguous run of tiles per workgroup: this workgroup's run [*t0, *t1) (false: it has
// none; the same answer for all its threads), and — by thread 0 into *s_first, which the caller's next barrier publishes — the first
// row of that run: the first i of [0, last] that is not before(i, x), x = t0 · T the run's first byte counted from the range's
// start.  `before` is monotone in i and false for `last`; it says what "the row lies in front of byte x" means to the caller.
template <typename Before>
__device__ __forceinline__ bool tile_run(int64_t ntiles, int T, int64_t last, Before before, int64_t* t0, int64_t* t1, long long* s_first) {
  const int64_t per = (ntiles + gridDim.x - 1) / gridDim.x;
  *t0 = (int64_t)blockIdx.x * per;
  *t1 = *t0 + per < ntiles ? *t0 + per : ntiles;
  if (*t0 >= *t1) return false;
  if (threadIdx.x == 0) {
    const int64_t x = *t0 * T;
    int64_t lo = 0, hi = last;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (before(mid, x)) lo = mid + 1;
      else hi = mid;
    }
    *s_first = lo;
  }
  return true;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
inline int tile_bytes(const ah_ctx* c) {   // (ah_ctx_set_option refuses values outside kMinTile … kMaxTile)
  const int t = c->opt_string_tile_bytes ? c->opt_string_tile_bytes : kDefaultTile;
  return t < kMinTile ? kMinTile : t > kMaxTile ? kMaxTile : t;
}
inline unsigned tile_grid(const ah_ctx* c) { return (unsigned)(c->num_cu > 0 ? c->num_cu : 1) * kWgPerCu; }
inline unsigned chunk_grid(ah_ctx* c, int64_t n) { return ah_stream_grid(c, ah_ceil_div(ah_ceil_div(n, 64), kBlock / 64), 8); }   // a wave per 64 rows

// the column of a string call; fixed_ok: fixed slots (offset_width 0) are taken
inline int check_column(ah_ctx* c, const char* fn, const ah_cmp_operand* o, int64_t n, bool fixed_ok) {
  if (n < 0) return ah_fail(c, AH_EINVALID, "%s: negative length", fn);
  if (!o) return ah_fail(c, AH_EINVALID, "%s: null operand descriptor", fn);
  if (o->offset_width == 0 && !fixed_ok) return ah_fail(c, AH_EINVALID, "%s: the column needs 4- or 8-byte offsets, not fixed slots", fn);
  if (o->offset_width != 0 && o->offset_width != 4 && o->offset_width != 8)
    return ah_fail(c, AH_EINVALID, "%s: offset width must be 0, 4 or 8 (got %d)", fn, o->offset_width);
  if (o->offset_width == 0 && o->byte_width < 0) return ah_fail(c, AH_EINVALID, "%s: negative byte width", fn);
  if (o->off < 0) return ah_fail(c, AH_EINVALID, "%s: negative element offset", fn);
  if (o->broadcast) return ah_fail(c, AH_EINVALID, "%s: the column cannot be a broadcast scalar", fn);
  if (n > 0 && o->offset_width != 0 && !o->offsets) return ah_fail(c, AH_EINVALID, "%s: null offsets", fn);
  return AH_OK;
}

}  // namespace
