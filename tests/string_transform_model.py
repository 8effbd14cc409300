"""The string transforms in plain Python, over lists of `bytes` / None (a null row): the range of its own bytes every row keeps, the
output rows, the output offsets.  Uses neither pyarrow nor the product; tests/test_string_transform_model_host.py pins it to pyarrow
on valid UTF-8, and on bytes that are no UTF-8 it is the definition the device is held to.

Code points: a byte that is not 10xxxxxx starts a code point, the continuation bytes behind it belong to it; the first byte of a row
starts one whatever it is."""
import numpy as np

WHOLE, SLICE_BYTES, SLICE_CODEPOINTS, TRIM_BYTES, TRIM_CODEPOINTS = 0, 1, 2, 3, 4
LEFT, RIGHT, BOTH = 1, 2, 3
WHITESPACE = b"\t\n\v\f\r "
UPPER = bytes(c - 32 if 97 <= c <= 122 else c for c in range(256))
LOWER = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


def code_point_starts(row):
    return [i for i, b in enumerate(row) if i == 0 or (b & 0xC0) != 0x80]


def code_points(row):
    starts = code_point_starts(row)
    return [bytes(row[s:e]) for s, e in zip(starts, starts[1:] + [len(row)])]


def row_range(row, op, start=0, stop=None, sides=BOTH, chars=b""):
    """→ (a, b): the row's result is row[a:b]"""
    n = len(row)
    if op == WHOLE:
        return 0, n
    if op == SLICE_BYTES:
        a, b, _ = slice(start, stop).indices(n)
        return a, max(a, b)
    if op == SLICE_CODEPOINTS:
        pos = code_point_starts(row) + [n]
        a, b, _ = slice(start, stop).indices(len(pos) - 1)
        return pos[a], pos[max(a, b)]
    if op == TRIM_BYTES:
        a, b = 0, n
        while sides & LEFT and a < b and row[a] in chars:
            a += 1
        while sides & RIGHT and b > a and row[b - 1] in chars:
            b -= 1
        return a, b
    if op == TRIM_CODEPOINTS:
        cps, members = code_points(row), set(code_points(chars))
        i, j = 0, len(cps)
        while sides & LEFT and i < j and cps[i] in members:
            i += 1
        while sides & RIGHT and j > i and cps[j - 1] in members:
            j -= 1
        return sum(len(c) for c in cps[:i]), sum(len(c) for c in cps[:j])
    raise ValueError(op)


def ranges(rows, op, **kw):
    """→ [(a, b) per row]; a null row keeps nothing: (0, 0)"""
    return [(0, 0) if r is None else row_range(r, op, **kw) for r in rows]


def transform(rows, op, byte_map=None, **kw):
    """→ the output rows (None stays None)"""
    out = []
    for r, (a, b) in zip(rows, ranges(rows, op, **kw)):
        out.append(None if r is None else (r[a:b] if byte_map is None else r[a:b].translate(byte_map)))
    return out


def offsets(out_rows, dtype=np.int32):
    """the output offsets: a null row has length 0"""
    o = np.zeros(len(out_rows) + 1, dtype)
    o[1:] = np.cumsum([0 if r is None else len(r) for r in out_rows], dtype=np.int64)
    return o


def payload(out_rows):
    return b"".join(r for r in out_rows if r is not None)


# the thirteen functions by name → (op, fixed keywords, byte map); slices take start / stop, the trims with characters take chars
FUNCTIONS = {
    "ascii_upper": (WHOLE, {}, UPPER),
    "ascii_lower": (WHOLE, {}, LOWER),
    "utf8_slice_codeunits": (SLICE_CODEPOINTS, {}, None),
    "binary_slice": (SLICE_BYTES, {}, None),
    "ascii_trim": (TRIM_BYTES, {"sides": BOTH}, None),
    "ascii_ltrim": (TRIM_BYTES, {"sides": LEFT}, None),
    "ascii_rtrim": (TRIM_BYTES, {"sides": RIGHT}, None),
    "ascii_trim_whitespace": (TRIM_BYTES, {"sides": BOTH, "chars": WHITESPACE}, None),
    "ascii_ltrim_whitespace": (TRIM_BYTES, {"sides": LEFT, "chars": WHITESPACE}, None),
    "ascii_rtrim_whitespace": (TRIM_BYTES, {"sides": RIGHT, "chars": WHITESPACE}, None),
    "utf8_trim": (TRIM_CODEPOINTS, {"sides": BOTH}, None),
    "utf8_ltrim": (TRIM_CODEPOINTS, {"sides": LEFT}, None),
    "utf8_rtrim": (TRIM_CODEPOINTS, {"sides": RIGHT}, None),
}
SLICES = ("utf8_slice_codeunits", "binary_slice")
TRIMS_WITH_CHARACTERS = ("ascii_trim", "ascii_ltrim", "ascii_rtrim", "utf8_trim", "utf8_ltrim", "utf8_rtrim")


def call(name, rows, **kw):
    op, fixed, byte_map = FUNCTIONS[name]
    return transform(rows, op, byte_map, **fixed, **kw)
