/* arrowhip_strings.h — the string predicates of libarrowhip_strings.so: substring, prefix / suffix, LIKE and lengths over
 * String / Binary / LargeString / LargeBinary columns.  A library of its own beside libarrowhip.so (whose entry-point list,
 * include/arrowhip.h, stays as it is): it works on the same ah_ctx — its stream, its scratch arena, its options — and takes its
 * columns as the ah_cmp_operand of the comparisons.  Link both; plain C. */
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
 * refused before anything is launched; n = 0 touches nothing.  No call synchronises with the host.
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

#ifdef __cplusplus
}
#endif
#endif /* ARROWHIP_STRINGS_H */
