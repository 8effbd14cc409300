"""The two entry points of ah_string_transform.hip through the C ABI against the host model (tests/string_transform_model.py, itself
pinned to pyarrow in tests/test_string_transform_model_host.py).  Every output — source starts, output offsets, data — sits in a
GuardedBuffer whose bands are read back after the call, and the comparison is byte for byte: nothing here has a tolerance.

The gather cuts the OUTPUT bytes into tiles of `string_tile_bytes` (T); with T = 64 or 333 a few hundred bytes put output rows on and
across tile borders and every tile in a workgroup of its own.  The ranges pass lets a lane look at 64 bytes of a row alone and hands
longer walks to the wave; the gather copies ≤ 64 bytes by the lane, ≤ 4096 by the wave, more by the workgroup (the last only with the
default tile: a smaller one clips every row below it)."""
import numpy as np
import pytest

from tests import string_transform_model as M
from tests.backends import GuardedBuffer

pytestmark = pytest.mark.gpu

TILES = (64, 333)
LANE_WALK = 64   # kLaneWalk of the kernel: where a row goes from its lane to the wave
FILL = 0xCD
E2, E3, E4 = "é".encode(), "€".encode(), "𝄞".encode()

# (name, op, keywords, byte map): what the thirteen functions ask of the pair, and a few more
OPS = [
    ("whole", M.WHOLE, {}, None),
    ("upper", M.WHOLE, {}, M.UPPER),
    ("lower", M.WHOLE, {}, M.LOWER),
    ("bytes[2:]", M.SLICE_BYTES, {"start": 2}, None),
    ("bytes[-70:-1]", M.SLICE_BYTES, {"start": -70, "stop": -1}, None),
    ("bytes[1:65]", M.SLICE_BYTES, {"start": 1, "stop": 65}, None),
    ("cp[0:2]", M.SLICE_CODEPOINTS, {"start": 0, "stop": 2}, None),
    ("cp[2:]", M.SLICE_CODEPOINTS, {"start": 2}, None),
    ("cp[-4:]", M.SLICE_CODEPOINTS, {"start": -4}, None),
    ("cp[3:-3]", M.SLICE_CODEPOINTS, {"start": 3, "stop": -3}, None),
    ("cp[-66:70]", M.SLICE_CODEPOINTS, {"start": -66, "stop": 70}, None),
    ("cp[5:1]", M.SLICE_CODEPOINTS, {"start": 5, "stop": 1}, None),
    ("trim ws", M.TRIM_BYTES, {"sides": M.BOTH, "chars": M.WHITESPACE}, None),
    ("ltrim ws", M.TRIM_BYTES, {"sides": M.LEFT, "chars": M.WHITESPACE}, None),
    ("rtrim ws", M.TRIM_BYTES, {"sides": M.RIGHT, "chars": M.WHITESPACE}, None),
    ("trim bytes", M.TRIM_BYTES, {"sides": M.BOTH, "chars": b"xa\xc3 "}, None),
    ("trim no bytes", M.TRIM_BYTES, {"sides": M.BOTH, "chars": b""}, None),
    ("utf8 trim", M.TRIM_CODEPOINTS, {"sides": M.BOTH, "chars": "x é𝄞".encode()}, None),
    ("utf8 ltrim", M.TRIM_CODEPOINTS, {"sides": M.LEFT, "chars": "€a ".encode()}, None),
    ("utf8 rtrim", M.TRIM_CODEPOINTS, {"sides": M.RIGHT, "chars": "b€é𝄞 ".encode()}, None),
    ("utf8 trim nothing", M.TRIM_CODEPOINTS, {"sides": M.BOTH, "chars": b""}, None),
]


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
    """rows (bytes, or None: a null whose slot holds junk bytes) on the device: `off` junk rows in front (the array offset), a first
    offset that is not 0, junk bytes behind the last row, and — where a row is None — a validity bitmap read from bit `voff` on"""

    def __init__(self, ctx, rows, ow=4, off=0, voff=0, rng=None):
        rng = rng or np.random.default_rng(0)
        junk = [bytes(rng.integers(97, 100, int(k), dtype=np.uint8)) for k in rng.integers(0, 6, off)]
        lead = bytes(rng.integers(97, 100, 3, dtype=np.uint8))
        slots = [bytes(rng.integers(32, 100, int(rng.integers(0, 5)), dtype=np.uint8)) if r is None else r for r in rows]
        allrows = junk + slots
        offsets = np.zeros(len(allrows) + 1, np.int32 if ow == 4 else np.int64)
        offsets[0] = len(lead)
        offsets[1:] = len(lead) + np.cumsum([len(r) for r in allrows], dtype=np.int64)
        data = np.frombuffer(lead + b"".join(allrows) + b"abcabcab", np.uint8)
        self.rows, self.n, self.ow, self.off, self.voff = list(rows), len(rows), ow, off, voff
        self.dtype = offsets.dtype
        self.slot_starts = offsets[off:off + self.n].astype(np.int64)
        self.keep = [ctx.to_device(offsets, pad=8), ctx.to_device(data, pad=16)]
        self.dev = (ow, 0, self.keep[0], self.keep[1], off)
        self.valid = None
        if any(r is None for r in rows):
            bits = rng.integers(0, 2, voff + self.n + 9).astype(np.uint8)   # junk bits in front and behind
            bits[voff:voff + self.n] = [r is not None for r in rows]
            self.keep.append(ctx.to_device(np.packbits(bits, bitorder="little"), pad=8))
            self.valid = self.keep[-1]


def guarded(ctx, nbytes, name):
    g = GuardedBuffer(ctx, nbytes, name=name)
    g.memset(FILL)
    return g


def run(ctx, col, op, byte_map=None, what="", **kw):
    """ah_string_ranges + ah_string_gather on the column, every output guarded → (total, data bytes); compared with the model"""
    what = str((what, op, {k: (v if not isinstance(v, bytes) else v[:12]) for k, v in kw.items()}, "map" if byte_map else "", "n", col.n, "ow", col.ow))
    w = col.ow
    starts, offs = guarded(ctx, col.n * w, "source starts"), guarded(ctx, (col.n + 1) * w, "output offsets")
    total = ctx.string_ranges(op, col.dev, col.n, starts, offs, start=kw.get("start", 0), stop=kw.get("stop"), sides=kw.get("sides", 3),
                              chars=kw.get("chars", b""), valid=col.valid, valid_offset=col.voff)
    starts.check(what)
    offs.check(what)
    want_ranges = M.ranges(col.rows, op, **kw)
    want_rows = M.transform(col.rows, op, byte_map, **kw)
    want_offsets = M.offsets(want_rows, col.dtype)
    got_offsets = offs.download(col.dtype, col.n + 1)
    assert got_offsets.tobytes() == want_offsets.tobytes(), (what, "offsets", np.flatnonzero(got_offsets != want_offsets)[:8].tolist())
    assert total == int(want_offsets[-1]), (what, "total", total, int(want_offsets[-1]))
    got_starts = starts.download(col.dtype, col.n).astype(np.int64)
    want_starts = col.slot_starts + np.array([a for a, _ in want_ranges], np.int64)
    kept = np.array([b > a for a, b in want_ranges], bool)   # (where an empty result starts is nobody's business, but it lies in the row's slot)
    assert (got_starts[kept] == want_starts[kept]).all(), (what, "source starts", np.flatnonzero(kept & (got_starts != want_starts))[:8].tolist())
    slot_ends = col.slot_starts + np.array([0 if r is None else len(r) for r in col.rows], np.int64)
    assert ((got_starts >= col.slot_starts) & (got_starts <= np.maximum(slot_ends, col.slot_starts))).all(), (what, "a source start outside its row")
    data = guarded(ctx, total, "output data")
    ctx.string_gather(col.dev, starts, offs, col.n, data, byte_map)
    ctx.sync()
    data.check(what)
    starts.check(what)
    offs.check(what)
    got = data.download(np.uint8, total).tobytes()
    want = M.payload(want_rows)
    if got != want:
        g, x = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        raise AssertionError((what, "data: first differing output bytes", np.flatnonzero(g != x)[:8].tolist(), "of", total))
    return total, got


def text(rng, k, alphabet=(b"a", b"b", b"x", b" ", b"\t", E2, E3, E4, b"Q", b"z")):
    """about k bytes of valid UTF-8 with 1- to 4-byte code points and trimmed characters in it"""
    out = b""
    while len(out) < k:
        out += alphabet[int(rng.integers(0, len(alphabet)))]
    return out


# ---- every op over rows that start, end and lie across tile borders ------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES, indirect=True)
@pytest.mark.parametrize("ow", (4, 8))
def test_every_op_over_rows_on_and_across_tile_borders(ctx, tile, ow):
    """rows of 0, 1, T − 1, T, T + 1 and 3 T bytes among short ones, valid UTF-8 cut so that it stays valid, nulls whose slots hold
    junk, `off` junk rows in front, a validity bit offset that is no multiple of 8"""
    rng = np.random.default_rng(tile + ow)
    T = tile
    rows = []
    for k in (0, 1, T - 1, T, T + 1, 3 * T, 5, 0, LANE_WALK - 1, LANE_WALK, LANE_WALK + 1, 2 * T + 3):
        body = text(rng, k)
        while len(body) > k:   # cut whole code points until it fits, then pad with a trimmed byte
            body = body[:M.code_point_starts(body)[-1]]
        rows.append(body + b" " * (k - len(body)))
        rows.append(None)
        rows.append(b" x" + body + b"\t ")
    col = Column(ctx, rows, ow=ow, off=5, voff=13, rng=rng)
    for name, op, kw, byte_map in OPS:
        run(ctx, col, op, byte_map, what=name, **kw)


# ---- a multi-byte code point swept over the lane-to-wave switch and a tile border ----------------------------------------------------------
@pytest.mark.parametrize("tile", TILES, indirect=True)
@pytest.mark.parametrize("cp", (E2, E3, E4), ids=("2-byte", "3-byte", "4-byte"))
def test_a_code_point_swept_across_the_wave_switch_and_a_tile_border(ctx, tile, cp):
    """row k holds one code point of 2 / 3 / 4 bytes at byte p_k among ASCII, p_k running over position 64 (where the lane hands the
    row to the wave) and over T (a tile border of the output), counted from the front and — the row reversed — from the back.  The
    slices start and stop one code point in front of it, on it and behind it."""
    T = tile
    ps = sorted(set(range(LANE_WALK - 6, LANE_WALK + 6)) | set(range(T - 6, T + 6)) | {2 * LANE_WALK - 1, 2 * LANE_WALK, 2 * LANE_WALK + 1})
    front = [b"a" * p + cp + b"b" * 9 for p in ps]
    back = [b"b" * 9 + cp + b"a" * p for p in ps]
    col = Column(ctx, front + back, ow=4, off=3)
    for p in ps:   # p ASCII code points in front of (behind) the swept one; every slice meets the rows of p − 1, p and p + 1 as well
        for start, stop in ((p, None), (0, p + 1), (1, p + 2), (-p - 1, None), (0, -p), (-p - 3, -p + 1)):
            run(ctx, col, M.SLICE_CODEPOINTS, what=("sweep", p), start=start, stop=stop)
    members = cp + b"ab"
    for sides in (M.LEFT, M.RIGHT, M.BOTH):
        run(ctx, col, M.TRIM_CODEPOINTS, what="sweep: all of it goes", sides=sides, chars=members)
        run(ctx, col, M.TRIM_CODEPOINTS, what="sweep: stops at the code point", sides=sides, chars=b"ab")
        run(ctx, col, M.TRIM_BYTES, what="sweep: stops at its second byte", sides=sides, chars=b"ab" + cp[:1])


# ---- row counts around the wave and the workgroup ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES, indirect=True)
@pytest.mark.parametrize("n", (1, 63, 64, 65, 257, 1025))
def test_row_counts(ctx, tile, n):
    rng = np.random.default_rng(n)
    rows = [None if rng.random() < 0.15 else b" " * int(rng.integers(0, 4)) + text(rng, int(rng.integers(0, 24))) + b" " * int(rng.integers(0, 4)) for _ in range(n)]
    for ow, off, voff in ((4, 0, 3), (8, 7, 0)):
        col = Column(ctx, rows, ow=ow, off=off, voff=voff, rng=rng)
        for name, op, kw, byte_map in (OPS[1], OPS[6], OPS[7], OPS[8], OPS[12], OPS[17]):
            run(ctx, col, op, byte_map, what=name, **kw)


# ---- the wave paths: one long row -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", (333, 0), indirect=True)
def test_long_rows_take_the_wave_paths(ctx, tile):
    """a row of 5000 bytes, rows of 5000 trimmed characters in front of / behind one kept byte, 2500 trimmed 2-byte code points; with
    the default tile (0) the 5000-byte rows are whole in one workgroup's run and are copied by the workgroup"""
    rng = np.random.default_rng(5)
    long_row = text(rng, 5000)
    rows = [b"ab", long_row, None, b" " * 5000 + b"k", b"k" + b" " * 5000, b" " * 5000, E2 * 2500 + b"k", b"k" + E2 * 2500, E2 * 2500, b"", b"tail"]
    col = Column(ctx, rows, ow=4, off=2, voff=5, rng=rng)
    for name, op, kw, byte_map in OPS:
        run(ctx, col, op, byte_map, what=name, **kw)
    for start, stop in ((-4000, None), (3000, 4500), (-4500, -3000), (2400, None), (0, 2499), (-1, None), (4999, None)):
        run(ctx, col, M.SLICE_CODEPOINTS, what="long", start=start, stop=stop)
    for sides in (M.LEFT, M.RIGHT, M.BOTH):
        run(ctx, col, M.TRIM_CODEPOINTS, what="long", sides=sides, chars=E2 + b" ")
        run(ctx, col, M.TRIM_BYTES, what="long", sides=sides, chars=E2 + b" ")


def test_long_rows_queued_in_a_late_iteration_of_a_run(ctx):
    """default tile: one workgroup's run holds 700 short rows — three iterations of its row walk without a queued row — and then rows
    of more than 4096 bytes, which its threads queue for the whole workgroup in the third iteration and the ones behind it; the
    last long row crosses into the next workgroup's run.  (Whether the queue holds a row is decided by a barrier reduction, not by a
    read of the slot counter.)"""
    ctx.set_option("string_tile_bytes", 0)
    rng = np.random.default_rng(77)
    rows = [text(rng, int(k)) for k in rng.integers(0, 12, 700)] + [text(rng, 4500), b"xy", text(rng, 5000)] + [text(rng, 3)] * 300 + [text(rng, 9000), b"", text(rng, 4097)]
    col = Column(ctx, rows, ow=4, off=1)
    assert sum(len(r) for r in rows[:700]) < 16384 - 4500
    for name, op, kw, byte_map in (OPS[0], OPS[1], OPS[3]):
        run(ctx, col, op, byte_map, what=name, **kw)


# ---- nothing to write ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES, indirect=True)
def test_a_column_of_nulls_writes_no_data(ctx, tile):
    col = Column(ctx, [None] * 130, ow=4, off=1, voff=9)
    for name, op, kw, byte_map in OPS:
        total, got = run(ctx, col, op, byte_map, what=name, **kw)
        assert total == 0 and got == b""
    empty = Column(ctx, [b""] * 70 + [b"  "] * 5, ow=8)
    assert run(ctx, empty, M.TRIM_BYTES, sides=M.BOTH, chars=b" ")[0] == 0


def test_no_rows_touch_nothing(ctx):
    col = Column(ctx, [b"abc"], ow=4)
    starts, offs, data = guarded(ctx, 8, "source starts"), guarded(ctx, 8, "output offsets"), guarded(ctx, 8, "output data")
    assert ctx.string_ranges(M.WHOLE, col.dev, 0, starts, offs) == 0
    ctx.string_gather(col.dev, starts, offs, 0, data)
    ctx.sync()
    for g in (starts, offs, data):
        g.check("n = 0")
        assert (g.download(np.uint8, 8) == FILL).all()


def test_bad_arguments_are_refused_before_any_launch(ctx):
    import arrow_go_amd as ah
    col = Column(ctx, [b"abc", b"de"], ow=4)
    starts, offs = guarded(ctx, 8, "source starts"), guarded(ctx, 12, "output offsets")
    for kw in ({"op": 5}, {"op": -1}, {"op": M.TRIM_BYTES, "sides": 0}, {"op": M.TRIM_BYTES, "sides": 4}, {"op": M.TRIM_BYTES, "chars": b"a" * 1025},
               {"op": M.TRIM_CODEPOINTS, "chars": b"\xff"}, {"op": M.TRIM_CODEPOINTS, "chars": b"\xe2\x82"}, {"op": M.WHOLE, "valid_offset": -1}, {"op": M.WHOLE, "n": -1}):
        kw = dict(kw)
        op, n = kw.pop("op"), kw.pop("n", 2)
        with pytest.raises(ah.ErrInvalid):
            ctx.string_ranges(op, col.dev, n, starts, offs, **kw)
    with pytest.raises(ah.ErrInvalid):
        ctx.string_ranges(M.WHOLE, (0, 3, None, col.keep[1], 0), 2, starts, offs)   # fixed slots
    with pytest.raises(ah.ErrInvalid):
        ctx.string_ranges(M.WHOLE, col.dev, 2, None, offs)
    ctx.sync()
    for g in (starts, offs):
        g.check("refused call")
        assert (g.download(np.uint8, 8) == FILL).all()


# ---- positions no Int32 holds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", (64,), indirect=True)
def test_positions_beyond_int32_on_a_large_string_column(ctx, tile):
    rng = np.random.default_rng(31)
    rows = [text(rng, int(k)) for k in rng.integers(0, 200, 40)] + [None, b""]
    col = Column(ctx, rows, ow=8, off=2, voff=1, rng=rng)
    big = 2**31
    for start, stop in ((-big - 5, big + 5), (big + 1, None), (-big - 1, None), (0, big * 4), (2, -big * 2), (-3, big + 7), (-2**63, 2**63 - 1), (2**63 - 1, None),
                        (-2**63, -2**63), (3, -2**63)):
        run(ctx, col, M.SLICE_CODEPOINTS, what="beyond int32", start=start, stop=stop)
        run(ctx, col, M.SLICE_BYTES, what="beyond int32", start=start, stop=stop)


# ---- bytes that are no UTF-8: the model alone is the yardstick -----------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES, indirect=True)
def test_invalid_utf8_follows_the_model(ctx, tile):
    """a lone continuation byte, one at the row's start, runs of them longer than a code point and longer than a wave's step, a lead
    byte cut off at the row's end, bytes that never occur in UTF-8"""
    pad = b"a" * 70
    rows = [b"\x80", b"a\x80b", b"\x80\x80ab", b"ab\xc3", b"ab\xe2\x82", b"ab\xf0\x9d\x84", b"\xc3", b"\xff\xfe", b"a" + b"\x80" * 6 + b"b", b"a" + b"\x80" * 200 + b"b",
            b"\x80" * 130, pad + b"\xe2\x82", pad + b"\x80" + pad, b"\xe2\x82" + pad, E3 + b"\x80" + E3, None, b"\xc3\xa9\xa9", pad + b"\xf0\x9d\x84\x9e\x80x" + pad]
    col = Column(ctx, rows, ow=4, off=1, voff=6)
    for start, stop in ((0, None), (1, None), (2, None), (-1, None), (-2, None), (0, 1), (0, -1), (1, -1), (70, None), (-71, None), (0, 71), (-72, 72), (3, 3)):
        run(ctx, col, M.SLICE_CODEPOINTS, what="invalid", start=start, stop=stop)
    for sides in (M.LEFT, M.RIGHT, M.BOTH):
        for chars in (b"a", b"ab", "a€".encode(), "é".encode(), b"", "ab𝄞".encode()):
            run(ctx, col, M.TRIM_CODEPOINTS, what="invalid", sides=sides, chars=chars)
        run(ctx, col, M.TRIM_BYTES, what="invalid", sides=sides, chars=b"a\x80\xff\xc3")
    run(ctx, col, M.WHOLE, M.UPPER, what="invalid")


# ---- the identity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", (64, 333, 0), indirect=True)
@pytest.mark.parametrize("ow", (4, 8))
def test_binary_slice_from_0_is_the_identity(ctx, tile, ow):
    rng = np.random.default_rng(tile * 2 + ow)
    rows = [bytes(rng.integers(0, 256, int(k), dtype=np.uint8)) for k in rng.integers(0, 90, 300)] + [bytes(rng.integers(0, 256, 9000, dtype=np.uint8)), b"", b"\x00"]
    col = Column(ctx, rows, ow=ow, off=4)
    total, got = run(ctx, col, M.SLICE_BYTES, what="identity", start=0, stop=None)
    assert got == b"".join(rows) and total == sum(len(r) for r in rows)
