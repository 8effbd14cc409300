/* arrowhip_string_transform.h — the string transforms of libarrowhip_string_transform.so: slice, trim and the ASCII case mappings
 * over String / Binary / LargeString / LargeBinary columns.  A third library beside libarrowhip.so and libarrowhip_strings.so
 * (whose entry-point lists, include/arrowhip.h and include/arrowhip_strings.h, stay as they are): it works on the same ah_ctx — its
 * stream, its arenas, its options — and takes its column as the ah_cmp_operand of the comparisons.  Link it with libarrowhip.so;
 * plain C. */
#ifndef ARROWHIP_STRING_TRANSFORM_H
#define ARROWHIP_STRING_TRANSFORM_H
#include "arrowhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- string transforms whose result is ONE CONTIGUOUS SUB-RANGE of the row's bytes (NEW — no reference analogue: arrow-go has none
 * of them; the semantics are Arrow C++'s utf8_slice_codeunits, binary_slice, ascii_trim*, utf8_trim*, ascii_upper / ascii_lower;
 * DESIGN.md §3.18) -----------------------------------------------------------------------------------------------------------------
 * Two calls with the caller's allocation in between, like ah_take_binary_offsets / ah_take_binary_data: ah_string_ranges computes
 * every row's range and the output offsets and brings the byte total home; ah_string_gather copies the bytes, optionally through a
 * byte map.  The column is an ah_cmp_operand with broadcast = 0 and 4- or 8-byte offsets; buffers are DEVICE memory, `chars` and
 * `map` HOST memory (pageable is fine) that the caller may reuse as soon as the call returns: `map` is read during the call and
 * travels to the kernel in its arguments; `chars` is turned into a table on the call's stack and uploaded, and ah_string_ranges
 * synchronises before it returns, also where it fails after the upload.  A bad argument (a null or misaligned output included) is
 * refused before anything is launched; n = 0 touches nothing.
 *
 * A null row (validity bit valid_offset + i clear; valid = NULL: no nulls) has length 0 in the output whatever its slot holds, its
 * source start is the slot's first byte.
 *
 * Code points: a byte that is not 10xxxxxx starts a code point, the continuation bytes behind it belong to it; the first byte of a
 * row starts one whatever it is.  Nothing is validated: on bytes that are no UTF-8 this rule is the definition. */
#define AH_STX_WHOLE 0            /* the whole row (the case mappings; the identity) */
#define AH_STX_SLICE_BYTES 1      /* Python's row[start:stop] over bytes; has_stop = 0: to the end of the row */
#define AH_STX_SLICE_CODEPOINTS 2 /* … over code points */
#define AH_STX_TRIM_BYTES 3       /* bytes of the set `chars` removed from the sides in `sides` */
#define AH_STX_TRIM_CODEPOINTS 4  /* … code points of the set `chars` (valid UTF-8, checked) */
#define AH_STX_LEFT 1
#define AH_STX_RIGHT 2
#define AH_STX_MAX_CHARS 1024     /* bytes of `chars` */
/* out_starts[i] (n values of the offset width) := the position in operand->data where row i's result starts;
 * out_offsets[0 … n] (the offset width) := the output offsets, out_offsets[0] = 0; *out_total_bytes_host := out_offsets[n].
 * The result of a row is never longer than the row, so 4-byte output offsets cannot overflow where the input's did not: there is no
 * overflow check.  Synchronises once, for the total.  start / stop / has_stop are read by the slices, sides / chars / chars_len by
 * the trims. */
int ah_string_ranges(ah_ctx* ctx, int op, int64_t start, int64_t stop, int has_stop, int sides, const uint8_t* chars, int64_t chars_len,
                     const ah_cmp_operand* operand, const uint8_t* valid, int64_t valid_offset, int64_t n, void* out_starts,
                     void* out_offsets, int64_t* out_total_bytes_host);
/* out_data[out_offsets[i] … out_offsets[i + 1]) := the bytes of operand->data from starts[i] on, each through map[byte] when `map`
 * (256 bytes) is given.  Work is cut by output bytes (context option "string_tile_bytes": 0 = 16384, else 64 … 32768; results never
 * depend on it): a long row is copied by every workgroup whose tiles it covers.  Every byte of [0, out_offsets[n]) has one writer,
 * nothing else is written.  No synchronisation. */
int ah_string_gather(ah_ctx* ctx, const ah_cmp_operand* operand, const void* starts, const void* out_offsets, int64_t n,
                     const uint8_t* map, uint8_t* out_data);

#ifdef __cplusplus
}
#endif
#endif /* ARROWHIP_STRING_TRANSFORM_H */
