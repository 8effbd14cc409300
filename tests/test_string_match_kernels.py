"""The four entry points of ah_string_match.hip through the C ABI against the host model (tests/string_match_model.py, itself pinned
to pyarrow in tests/test_string_match_model_host.py).  Every output sits in a GuardedBuffer whose bands are read back after the call,
and the comparison is byte for byte: nothing here has a tolerance.

The searches cut the value bytes into tiles of `string_tile_bytes` (T); most tests set T = 256 or 333 so that a few hundred bytes
put rows, matches and pattern windows on and across tile borders.  Rows of 3 T bytes start on a tile border (the tiles count from the
first row's first byte), so a plant at byte p of such a row sits at a known distance from the borders at T and 2 T."""
import numpy as np
import pytest

from tests import string_match_model as M
from tests.backends import GuardedBuffer

pytestmark = pytest.mark.gpu

SUBSTRING, STARTS_WITH, ENDS_WITH, EQUALS = 0, 1, 2, 3
TILES = (256, 333)
PATTERN_LENGTHS = (1, 2, 7, 8, 9, 16, 17, 63, 64, 65, 300)   # 300: longer than the tile
FILL = 0xCD
LIKE_PATTERNS = ["%", "%%", "_", "a%", "%a", "%a%b%", "a_c", "_%_", "\\%", "\\_", "a\\", "", "%é_", "a%%b", "__", "%_%_%", "_%", "%__", "a%b", "ab",
                 "%ab", "ab%", "%ab%", "a\\%c", "a\\bc", "é", "_é%", "%b_", "a_%_c", "%a_c%b", "%a\\bc%", "%a\\", "x" * 50, "%b%" + "_" * 45, "%ab_ab%ba_%"]


@pytest.fixture(scope="module")
def ctx():
    import arrow_go_amd as ah
    with ah.Context(0) as c:
        yield c
        c.set_option("string_tile_bytes", 0)


@pytest.fixture
def tile(ctx, request):
    ctx.set_option("string_tile_bytes", request.param)
    yield request.param
    ctx.set_option("string_tile_bytes", 0)


class Column:
    """rows on the device: `off` junk rows in front (the array offset), a first offset that is not 0, junk bytes behind the last row"""

    def __init__(self, ctx, rows, ow=4, off=0, rng=None):
        rng = rng or np.random.default_rng(0)
        junk = [bytes(rng.integers(97, 100, int(k), dtype=np.uint8)) for k in rng.integers(0, 6, off)]
        lead = bytes(rng.integers(97, 100, 3, dtype=np.uint8))
        allrows = junk + list(rows)
        lens = np.array([len(r) for r in allrows], np.int64)
        offsets = np.zeros(len(allrows) + 1, np.int32 if ow == 4 else np.int64)
        offsets[0] = len(lead)
        offsets[1:] = len(lead) + np.cumsum(lens)
        data = np.frombuffer(lead + b"".join(allrows) + b"abcabcab", np.uint8)
        self.rows, self.n, self.ow, self.off = list(rows), len(rows), ow, off
        self.keep = (ctx.to_device(offsets, pad=8), ctx.to_device(data, pad=16))
        self.dev = (ow, 0, self.keep[0], self.keep[1], off)


def guarded(ctx, nbytes, name, fill=None):
    g = GuardedBuffer(ctx, nbytes, name=name)
    if fill is None:
        g.memset(FILL)
    else:
        g.upload(fill)
    return g


def check_match(ctx, col, op, pattern, bit_off=0, what=""):
    want_flags = {SUBSTRING: M.match_substring, STARTS_WITH: M.starts_with, ENDS_WITH: M.ends_with, EQUALS: M.equals}[op](col.rows, pattern)
    check_bits(ctx, col, want_flags, bit_off, lambda out: ctx.string_match(op, col.dev, col.n, pattern, out, bit_off), ("ah_string_match", op, len(pattern), bit_off, what))


def check_like(ctx, col, utf8, pattern, bit_off=0, what=""):
    from arrow_go_amd import compute as ac
    want_flags = M.match_like(col.rows, pattern, utf8)
    program = ac.like_compile(pattern)
    check_bits(ctx, col, want_flags, bit_off, lambda out: ctx.string_like(col.dev, col.n, utf8, program, out, bit_off), ("ah_string_like", pattern, utf8, bit_off, what))


def check_bits(ctx, col, want_flags, bit_off, call, what):
    nbytes = (bit_off + col.n + 7) // 8 + 1
    before = np.random.default_rng(col.n + bit_off).integers(0, 256, nbytes, dtype=np.uint8)   # the neighbouring bits must survive
    out = guarded(ctx, nbytes, "bitmap", fill=before)
    call(out)
    ctx.sync()
    out.check(str(what))
    got = out.download(np.uint8, nbytes)
    want = before.copy()
    packed = M.pack(want_flags, bit_off, before)
    want[:len(packed)] = packed
    if got.tobytes() != want.tobytes():
        g = np.unpackbits(got, bitorder="little")[bit_off:bit_off + col.n]
        bad = np.flatnonzero(g != want_flags)
        raise AssertionError((what, "rows", bad[:8].tolist(), "or bits outside the range changed" if bad.size == 0 else ""))


def check_find(ctx, col, pattern, width=None, what=""):
    width = width or col.ow
    dtype = np.int32 if width == 4 else np.int64
    out = guarded(ctx, col.n * width, "find output")
    ctx.string_find(col.dev, col.n, pattern, width, out)
    ctx.sync()
    out.check(str(("ah_string_find", what)))
    got = out.download(dtype, col.n)
    want = M.find_substring(col.rows, pattern, dtype)
    assert got.tobytes() == want.tobytes(), ("ah_string_find", len(pattern), what, np.flatnonzero(got != want)[:8].tolist())


def check_length(ctx, col, utf8, width=None, what=""):
    width = width or col.ow
    dtype = np.int32 if width == 4 else np.int64
    out = guarded(ctx, col.n * width, "length output")
    ctx.string_length(col.dev, col.n, utf8, width, out)
    ctx.sync()
    out.check(str(("ah_string_length", utf8, what)))
    got = out.download(dtype, col.n)
    want = (M.utf8_length if utf8 else M.binary_length)(col.rows, dtype)
    assert got.tobytes() == want.tobytes(), ("ah_string_length", utf8, what, np.flatnonzero(got != want)[:8].tolist())


def the_pattern(m):
    return (b"abbabaab" * (m // 8 + 1))[:m - 1] + b"c" if m > 1 else b"c"   # ends in a byte the filler does not have


def filler(rng, k):
    return bytes(rng.choice(np.frombuffer(b"abxy", np.uint8), k))


# ---- one planted match swept across two consecutive tile borders ------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES, indirect=True)
@pytest.mark.parametrize("m", PATTERN_LENGTHS)
def test_a_match_at_every_position_across_two_tile_borders(ctx, tile, m):
    """rows of 3 T bytes, row k with the pattern planted at byte p_k: p runs from where the match ends in front of the border at T to
    where it starts behind the border at 2 T — every way a match can straddle, touch or clear a border.  One row without a plant."""
    rng = np.random.default_rng(m)
    T, pat = tile, the_pattern(m)
    rows = []
    for p in range(max(0, T - m - 1), min(2 * T + 1, 3 * T - m) + 1):
        r = bytearray(filler(rng, 3 * T))
        r[p:p + m] = pat
        rows.append(bytes(r))
    rows.append(filler(rng, 3 * T))
    for ow, off in ((4, 0), (8, 5)):
        col = Column(ctx, rows, ow, off, rng)
        check_match(ctx, col, SUBSTRING, pat, what=("sweep", T, ow, off))
        check_find(ctx, col, pat, what=("sweep", T, ow, off))


@pytest.mark.parametrize("tile", TILES, indirect=True)
def test_one_long_row_alone(ctx, tile):
    """the issue's own shape: ONE row of many tiles, the plant moved call by call over the border at 2 T (a handful of positions; the
    sweep above covers every position in one call)"""
    rng = np.random.default_rng(5)
    T, pat = tile, the_pattern(9)
    for p in (2 * T - 10, 2 * T - 9, 2 * T - 8, 2 * T - 1, 2 * T, 5 * T - 9):
        r = bytearray(filler(rng, 5 * T))
        r[p:p + 9] = pat
        col = Column(ctx, [bytes(r)], 4, 0, rng)
        check_match(ctx, col, SUBSTRING, pat, what=("alone", T, p))
        check_find(ctx, col, pat, what=("alone", T, p))
        check_length(ctx, col, True, what=("alone", T, p))


# ---- short rows packed around the borders ------------------------------------------------------------------------------------------------
def short_rows(rng, count, alphabet, max_len=40):
    pieces = [a.encode() for a in alphabet]
    rows = []
    for k in rng.integers(0, max_len + 1, count):
        r = b""
        while len(r) < k:
            r += pieces[int(rng.integers(0, len(pieces)))]
        rows.append(r)
    return rows


@pytest.mark.parametrize("tile", TILES, indirect=True)
@pytest.mark.parametrize("ow,off", [(4, 0), (4, 5), (8, 0), (8, 5)])
def test_rows_of_0_to_40_bytes_around_the_borders(ctx, tile, ow, off):
    rng = np.random.default_rng(tile + ow + off)
    rows = short_rows(rng, 700, ["a", "b", "ab", "c", "é", "日", "\n", "%", "_"])   # ≈ 14 000 bytes: some fifty tiles
    col = Column(ctx, rows, ow, off, rng)
    for pat in (b"a", b"ab", b"aba", "é".encode(), b"\xa9", "日a".encode(), b"abababab", b"babababab", rows[3][:17] or b"q"):
        check_match(ctx, col, SUBSTRING, pat, what=("short", tile))
        check_find(ctx, col, pat, what=("short", tile))
        for op in (STARTS_WITH, ENDS_WITH, EQUALS):
            check_match(ctx, col, op, pat, what=("short", tile))
    check_length(ctx, col, True, what=("short", tile))
    check_length(ctx, col, False, what=("short", tile))
    if ow == 4:
        check_find(ctx, col, b"ab", width=8, what="int64 output over 4-byte offsets")
        check_length(ctx, col, True, width=8, what="int64 output over 4-byte offsets")


@pytest.mark.parametrize("tile", (256,), indirect=True)
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_row_counts_and_bit_offsets(ctx, tile, n):
    rng = np.random.default_rng(n)
    rows = short_rows(rng, n, ["a", "b", "ab", "c"], max_len=12)
    col = Column(ctx, rows, 4, 5, rng)
    for bit_off in (0, 1, 3, 7):
        check_match(ctx, col, SUBSTRING, b"ab", bit_off, what=n)
        check_match(ctx, col, STARTS_WITH, b"ab", bit_off, what=n)
        check_match(ctx, col, SUBSTRING, b"", bit_off, what=n)     # the empty pattern: every row
        check_like(ctx, col, True, b"%a_b%", bit_off, what=n)
        check_like(ctx, col, True, b"%ab", bit_off, what=n)         # (a program the suffix predicate answers)
    check_match(ctx, col, EQUALS, b"", what=n)
    check_find(ctx, col, b"", what=n)
    check_find(ctx, col, b"ba", what=n)
    check_length(ctx, col, True, what=n)
    check_length(ctx, col, False, what=n)


def test_a_column_without_bytes(ctx):
    col = Column(ctx, [b""] * 300, 4, 5)
    check_match(ctx, col, SUBSTRING, b"a")
    check_find(ctx, col, b"a")
    check_length(ctx, col, True)
    check_like(ctx, col, True, b"%a_%")
    check_like(ctx, col, True, b"")


# ---- long patterns at the row edges (the whole-wave compare) -----------------------------------------------------------------------------
@pytest.mark.parametrize("m", [63, 64, 65, 72, 300, 4096])
def test_prefix_suffix_equals_with_long_patterns(ctx, m):
    rng = np.random.default_rng(m)
    pat = filler(rng, m)
    last_differs = pat[:-1] + b"q"
    rows = [pat, pat + b"x", b"x" + pat, pat[:-1], last_differs, pat + pat, b"", filler(rng, m), b"zz" + pat + b"zz"] * 9
    col = Column(ctx, rows, 8, 5, rng)
    for op in (STARTS_WITH, ENDS_WITH, EQUALS):
        check_match(ctx, col, op, pat, bit_off=3, what=m)


# ---- the first of several occurrences -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES, indirect=True)
def test_find_returns_the_first_occurrence(ctx, tile):
    rng = np.random.default_rng(3)
    T = tile
    long_aa = b"x" * (T - 1) + b"aaaa" + b"x" * T + b"aa"      # overlapping occurrences across the border at T, another two tiles on
    rows = [b"aaaa", b"aa", b"a", b"xaaxaa", b"ab" * 200, long_aa, b"x" * (2 * T) + b"aa" + b"x" * T + b"aa", b"aab" * 300]
    col = Column(ctx, rows, 4, 5, rng)
    for pat in (b"aa", b"a", b"aaa", b"ab", b"ba", b"aab"):
        check_find(ctx, col, pat, what=("first", T))
        check_match(ctx, col, SUBSTRING, pat, what=("first", T))


# ---- a row longer than the default tile among short ones ---------------------------------------------------------------------------------
def test_one_long_row_among_3000_short_ones_at_the_default_tile(ctx):
    ctx.set_option("string_tile_bytes", 0)
    rng = np.random.default_rng(8)
    rows = short_rows(rng, 3000, ["a", "b", "ab", "é", "x"], max_len=24)
    pat = the_pattern(17)
    long_row = bytearray(("é".encode() * 25000)[:40001] + filler(rng, 9000))   # 49 001 bytes: three tiles and a bit, half of it two-byte characters
    long_row[16384 - 5 - 7:16384 - 5 - 7 + 17] = pat                            # over the first border of the ROW'S OWN bytes (wherever the tiles fall) …
    long_row[-17:] = pat                                                        # … and at its very end
    rows.insert(1500, bytes(long_row))
    col = Column(ctx, rows, 4, 5, rng)
    check_match(ctx, col, SUBSTRING, pat, what="long row")
    check_find(ctx, col, pat, what="long row")
    check_find(ctx, col, b"ab", what="long row")
    check_match(ctx, col, ENDS_WITH, pat, what="long row")
    check_length(ctx, col, True, what="long row")
    check_length(ctx, col, False, what="long row")
    for like in (b"%a_b%", "%é_é%".encode() + pat, b"_%" + pat, b"%" + pat[:5] + b"%" + pat[-3:], "é%x_".encode()):
        check_like(ctx, col, True, like, what="long row")
        check_like(ctx, col, False, like, what="long row")


# ---- LIKE ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", (0, 256, 333), indirect=True)
@pytest.mark.parametrize("utf8", [True, False])
def test_like_patterns(ctx, tile, utf8):
    """the pattern list of the host test on a UTF-8 and a Binary view of the same bytes: rows shorter and longer than what a lane
    matches alone (256 bytes), than a tile, and than a tile with its overlap"""
    rng = np.random.default_rng(21)
    rows = short_rows(rng, 500, ["a", "b", "c", "ab", "%", "_", "\\", "é", "\n", "日", "x"], max_len=30)
    rows += ["héllo\nx".encode(), b"h_llo", b"a%c", b"a\\", b"a_c", "aéc".encode(), b"ab" * 30, b"ab" * 30 + b"c", b"a", b""]
    rows += short_rows(rng, 12, ["a", "b", "ab", "é", "x", "c"], max_len=1500)
    rows += [b"a" + b"x" * 700 + b"b" + "é".encode() * 200 + b"c", b"x" * 1000 + b"ab_ab" + b"y" * 300 + b"bacd"]
    col = Column(ctx, rows, 4, 5, rng)
    for pat in LIKE_PATTERNS:
        check_like(ctx, col, utf8, pat.encode(), what=tile)
    if not utf8:
        col = Column(ctx, [b"h\xffllo", b"h\xc3\xa9llo", b"\x80\x80", b"a\xc3", b"\xa9c"], 8, 0, rng)
        for pat in (b"h_llo", b"h__llo", b"__", b"a_", b"_c", b"%\x80"):
            check_like(ctx, col, False, pat, what="bytes that are no UTF-8")


# ---- refusals launch nothing ---------------------------------------------------------------------------------------------------------------
def test_refusals_and_empty_calls_touch_nothing(ctx):
    import arrow_go_amd as ah
    from arrow_go_amd import compute as ac
    col = Column(ctx, [b"abc", b"", b"xab"], 4, 5)
    fixed = (0, 3, None, col.keep[1], 0)
    out = guarded(ctx, 64, "untouched output")

    def refused(fn, match):
        with pytest.raises(ah.ErrInvalid, match=match):
            fn()

    refused(lambda: ctx.string_match(SUBSTRING, col.dev, -1, b"a", out), "negative length")
    refused(lambda: ctx.string_match(4, col.dev, 3, b"a", out), "bad op")
    refused(lambda: ctx.string_match(-1, col.dev, 3, b"a", out), "bad op")
    refused(lambda: ctx.string_match(SUBSTRING, fixed, 3, b"a", out), "needs 4- or 8-byte offsets")
    refused(lambda: ctx.string_find(fixed, 3, b"a", 4, out), "needs 4- or 8-byte offsets")
    refused(lambda: ctx.string_like(fixed, 3, True, ac.like_compile("a_"), out), "needs 4- or 8-byte offsets")
    refused(lambda: ctx.string_length(fixed, 3, True, 4, out), "needs 4- or 8-byte offsets")
    refused(lambda: ctx.string_match(SUBSTRING, col.dev, 3, b"a" * 4097, out), "pattern length 4097")
    refused(lambda: ctx.string_find(col.dev, 3, b"a" * 4097, 4, out), "pattern length 4097")
    refused(lambda: ctx.string_find(col.dev, 3, b"a", 2, out), "output width")
    refused(lambda: ctx.string_find((8,) + col.dev[1:], 3, b"a", 4, out), "8-byte output")
    refused(lambda: ctx.string_like(col.dev, 3, True, b"\x00\x01", out), "program")
    refused(lambda: ctx.string_like(col.dev, 3, True, bytes([0, 1, 0, 2, 0, 0, 97]), out), "truncated program")
    refused(lambda: ctx.string_like(col.dev, 3, True, bytes([8, 0, 0]), out), "unknown program flags")
    refused(lambda: ctx.string_like(col.dev, 3, True, ac.like_compile("_" * 2049), out), "at most 2048")
    refused(lambda: ctx.set_option("string_tile_bytes", 63), "string_tile_bytes")
    refused(lambda: ctx.set_option("string_tile_bytes", 32769), "string_tile_bytes")
    # n = 0: accepted, nothing written — also with null buffers
    ctx.string_match(SUBSTRING, col.dev, 0, b"a", out, 3)
    ctx.string_find(col.dev, 0, b"a", 4, out)
    ctx.string_like(col.dev, 0, True, ac.like_compile("a_%"), out, 3)
    ctx.string_length(col.dev, 0, True, 4, out)
    ctx.string_match(SUBSTRING, (4, 0, None, None, 0), 0, b"a", None)
    ctx.sync()
    out.check("refusals")
    assert out.download(np.uint8, 64).tobytes() == bytes([FILL]) * 64
    # FixedSizeBinary lengths: the slot width
    lens = guarded(ctx, 12, "fixed lengths")
    ctx.string_length(fixed, 3, False, 4, lens)
    ctx.sync()
    lens.check("fixed lengths")
    assert lens.download(np.int32, 3).tolist() == [3, 3, 3]
