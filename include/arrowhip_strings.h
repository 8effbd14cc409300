/* arrowhip_strings.h — the string entry points of libarrowhip.so: the predicates (substring, prefix / suffix, LIKE, lengths) and the
 * transforms (slice, trim, the ASCII case mappings) over String / Binary / LargeString / LargeBinary columns.  They are exports of
 * libarrowhip.so like those of include/arrowhip.h and work on the same ah_ctx — its stream, its arenas, its options —; their
 * columns are the ah_cmp_operand of the comparisons.  A header of their own because the Go binding covers include/arrowhip.h
 * entry for entry and does not bind these yet.  Plain C. */
#ifndef ARROWHIP_STRINGS_H
#define ARROWHIP_STRINGS_H
#include "arrowhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- string predicates: substring, prefix / suffix, LIKE, lengths (NEW — no reference analogue: arrow-go has none of them; the
 * semantics are Arrow C++'s match_substring, starts_with, ends_with, find_substring, match_like, binary_length, utf8_length;
 * DESIGN.md §3.17) -------------------------------------------------------------------------------------------------------------
 * The column is an ah_cmp_operand with broadcast = 0: String / Binary / LargeString / LargeBinary (offset_width 4 or 8); the
 * pattern calls refuse fixed slots, ah_string_length takes them.  Every row is computed, null slots included (the caller owns the
 * validity).  `pattern` / `program` are HOST memory, copied by the call; at most AH_STR_MAX_PATTERN bytes.  A bad argument (a
 * negative n, an unknown op, a fixed-width column where there must be offsets, a pattern over the limit, a malformed program) is
 * refused before anything is launched; n = 0 touches nothing.  None of these four calls synchronises with the host.
 *
 * The searches (substring, find, LIKE's `%lit%`, utf8 length) work over the value BYTES, not over rows: a workgroup stages a tile
 * of the data buffer in LDS (context option "string_tile_bytes": 0 = 16384, else 64 … 32768; results never depend on it), tests
 * every byte position of the tile in parallel and reduces per row; a row that reaches over a tile border is combined from its
 * tiles, its result written once. */
#define AH_STR_SUBSTRING 0   /* the pattern occurs in the row; the empty pattern matches every row */
#define AH_STR_STARTS_WITH 1
#define AH_STR_ENDS_WITH 2
#define AH_STR_EQUALS 3      /* the row is the pattern (what LIKE without a wildcard asks) */
#define AH_STR_MAX_PATTERN 4096
/* bits [out_bit_offset, out_bit_offset + n) of out_bits := the predicate of every row; every other bit is kept */
int ah_string_match(ah_ctx* ctx, int op, const ah_cmp_operand* operand, int64_t n, const uint8_t* pattern, int64_t pattern_len,
                    uint8_t* out_bits, int64_t out_bit_offset);
/* out[i] = the byte index of the pattern's first occurrence in row i, -1 if there is none, 0 for the empty pattern; out_width 4
 * (Int32) or 8 (Int64), 8 for a column with 8-byte offsets */
int ah_string_find(ah_ctx* ctx, const ah_cmp_operand* operand, int64_t n, const uint8_t* pattern, int64_t pattern_len, int out_width,
                   void* out);
/* SQL LIKE over the whole row, the pattern compiled on the host (arrow_go_amd/host/like_program.h, ahc_like_compile) into
 * `program`: byte 0 flags (AH_LIKE_*), bytes 1-2 the number of segments (little-endian), then per segment a 2-byte element count
 * and 2 bytes per element: {0, b} the literal byte b, {1, 0} one character (`_`).  Segments are what `%` separates; the first is
 * tied to the row's start with AH_LIKE_ANCHOR_START, the last to its end with AH_LIKE_ANCHOR_END, the others match at their first
 * occurrence behind the one before (leftmost-greedy, exact for LIKE).  utf8 != 0: `_` is one code point — a byte that is not
 * 10xxxxxx and the continuation bytes behind it —, else one byte.  Programs one simpler predicate answers (`%lit%`, `lit%`,
 * `%lit`, `lit`, `%`) run as ah_string_match does.  Output as ah_string_match.  What Arrow does with `\` is the compiler's business. */
#define AH_LIKE_ANCHOR_START 1
#define AH_LIKE_ANCHOR_END 2
int ah_string_like(ah_ctx* ctx, const ah_cmp_operand* operand, int64_t n, int utf8, const uint8_t* program, int64_t program_len,
                   uint8_t* out_bits, int64_t out_bit_offset);
/* out[i] = the bytes of row i (utf8 = 0; fixed slots allowed) or its code points = the bytes that are not 10xxxxxx (utf8 != 0;
 * what that counts on invalid UTF-8 is this rule's); out_width as ah_string_find */
int ah_string_length(ah_ctx* ctx, const ah_cmp_operand* operand, int64_t n, int utf8, int out_width, void* out);

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
#endif /* ARROWHIP_STRINGS_H */
