"""The six entry points of ah_conditional.hip through the C ABI against the host model (tests/conditional_model.py, itself pinned
against pyarrow in tests/test_conditional_model_host.py).  Every output sits in a GuardedBuffer whose two bands are read back after
every call, and the comparison with the model is byte for byte: no tolerance occurs anywhere in this feature.

ah_if_else: a lane holds V = 16 / width rows per step (one row of a 16- or 32-byte slot), a wave 64 V, a workgroup
B = kBlock * kUnroll * V (read from the source); widths the vector path does not take (3) go a row per lane, 64 per wave, kBlock
per workgroup step.  Row counts 0, 1, 7, 8, 9, 63, 64, 65, B - 1, B, B + 1, 3 B + 17 for the widths 1, 2, 3, 4, 8, 16, 32; the
three bit offsets drawn independently from {0, 3, 69}; each side with a bitmap or without, as an array or a broadcast row; the
condition all true, all false, all null and random; the value output at the sixteen phases of a 16-byte line (width 1).
The fills: S = kCarryRows, the rows of one workgroup of the carry's passes: row counts 0, 1, 63, 64, 65, S - 1, S, S + 1,
3 S + 17, the layouts below, both directions, validity offsets 0, 3, 69."""
import itertools
import os
import re

import numpy as np
import pytest

from tests import conditional_model as CM
from tests.backends import GuardedBuffer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "arrow_go_amd", "csrc", "ah_conditional.hip")).read()
K_BLOCK = int(re.search(r"constexpr int kBlock = (\d+);", _SRC).group(1))
K_UNROLL = int(re.search(r"constexpr int kUnroll = (\d+);", _SRC).group(1))
S = int(re.search(r"constexpr int kCarryRows = (\d+);", _SRC).group(1))
assert re.search(r"constexpr int V = W <= 16 \? 16 / W : 1;", _SRC), "the rows of a lane's step are no longer 16 / width"
VECTOR_WIDTHS = (1, 2, 4, 8, 16, 32)
WIDTHS = (1, 2, 3, 4, 8, 16, 32)
OFFSETS = (0, 3, 69)
FILL = 0xCD   # what an output holds before the call: a byte the kernel does not write shows


def rows_per_thread(w):
    return max(1, 16 // w) if w in VECTOR_WIDTHS else 1


def rows_per_wave(w):
    return 64 * rows_per_thread(w)


def rows_per_workgroup(w):
    return K_BLOCK * K_UNROLL * rows_per_thread(w) if w in VECTOR_WIDTHS else K_BLOCK


def sizes(b):
    return [0, 1, 7, 8, 9, 63, 64, 65, b - 1, b, b + 1, 3 * b + 17]


@pytest.fixture(scope="module")
def ctx():
    import arrow_go_amd as ah
    with ah.Context(0) as c:
        yield c


# ---- building the operands ----------------------------------------------------------------------------------------------------------
def bitmap_of(flags, off, rng):
    """flags at bits off …, random bits in front and behind (up to the byte's end and one more byte)"""
    total = off + len(flags)
    raw = rng.random(((total + 7) // 8 + 1) * 8) < 0.5
    raw[off:total] = flags
    return np.packbits(raw, bitorder="little")


class Cond:
    def __init__(self, ctx, kind, n, off, rng):
        data = {"true": np.ones(n, bool), "false": np.zeros(n, bool)}.get(kind, rng.random(n) < 0.5)
        valid = np.zeros(n, bool) if kind == "null" else (rng.random(n) < 0.9 if kind == "random_nulls" else None)
        self.off = off
        self.m_data = bitmap_of(data, off, rng)
        self.m_valid = None if valid is None else bitmap_of(valid, off, rng)
        self.d_data = ctx.to_device(self.m_data, pad=8)
        self.d_valid = None if valid is None else ctx.to_device(self.m_valid, pad=8)

    def dev(self):
        return self.d_data, self.d_valid, self.off

    def model(self):
        return self.m_data, self.m_valid, self.off


class Side:
    """one side on the device and as the model's tuple.  kind: "fixed" (w bytes), "bool", "binary" (ow 4 / 8, `lengths` drawn per row)"""

    def __init__(self, ctx, kind, n, off, has_valid, broadcast, rng, w=0, ow=0, lengths=None, scalar_valid=True):
        rows = off + (1 if broadcast else n)
        flags = rng.random(rows) < 0.8
        if broadcast:
            flags[off] = scalar_valid
        self.valid = bitmap_of(flags[off:], off, rng) if has_valid else None
        offsets = None
        if kind == "fixed":
            data = rng.integers(1, 256, max(rows * w, 1), dtype=np.uint8)   # never a zero byte: a null slot's payload must be MADE zero
        elif kind == "bool":
            data = bitmap_of(rng.random(rows - off) < 0.5, off, rng)
        else:
            lens = np.concatenate([rng.integers(0, 5, off), lengths[:rows - off]]).astype(np.int64)
            offsets = np.zeros(rows + 1, np.int32 if ow == 4 else np.int64)
            offsets[1:] = np.cumsum(lens)
            data = rng.integers(1, 256, max(int(offsets[-1]), 1), dtype=np.uint8)
        self.keep = [ctx.to_device(data, pad=16), None if offsets is None else ctx.to_device(offsets, pad=8),
                     None if self.valid is None else ctx.to_device(self.valid, pad=8)]
        self.dev = (ow, w, self.keep[1], self.keep[0], self.keep[2], off, int(broadcast))
        self.model = (ow, w, offsets, data, self.valid, off, int(broadcast))


def guarded(ctx, nbytes, name, lead=0):
    g = GuardedBuffer(ctx, nbytes, lead=lead, name=name)
    g.memset(FILL)
    return g


def check_bytes(got, want, what):
    assert got.tobytes() == np.asarray(want).tobytes(), what


# ---- ah_if_else ------------------------------------------------------------------------------------------------------------------------
COND_KINDS = ("true", "false", "null", "random", "random_nulls")


def run_if_else(ctx, n, w, cond_kind, offs, lvalid, rvalid, lbroad, rbroad, rng, lead=0, scalar_valid=True):
    cond = Cond(ctx, cond_kind, n, offs[0], rng)
    left = Side(ctx, "fixed", n, offs[1], lvalid, lbroad, rng, w=w, scalar_valid=scalar_valid)
    right = Side(ctx, "fixed", n, offs[2], rvalid, rbroad, rng, w=w)
    want_values, want_valid = CM.if_else(*cond.model(), left.model, right.model, n)
    out = guarded(ctx, n * w, "if_else values", lead=lead)
    ov = None if want_valid is None else guarded(ctx, (n + 7) // 8, "if_else validity")
    ctx.if_else(*cond.dev(), left.dev, right.dev, n, out, ov)
    ctx.sync()
    what = ("ah_if_else", n, w, cond_kind, offs, lvalid, rvalid, lbroad, rbroad, lead)
    out.check(str(what))
    check_bytes(out.download(np.uint8, n * w), want_values, what)
    if ov is not None:
        ov.check(str(what))
        check_bytes(ov.download(np.uint8, (n + 7) // 8), want_valid, what)


@pytest.mark.parametrize("w", WIDTHS)
def test_if_else_every_row_count(ctx, w):
    rng = np.random.default_rng(w)
    options = itertools.cycle(itertools.product(COND_KINDS, (True, False), (False, True), (False, True), (False, True)))
    offsets = itertools.cycle(itertools.product(OFFSETS, OFFSETS, OFFSETS))
    for n in sizes(rows_per_workgroup(w)):
        for _ in range(6):   # the options rotate through the row counts: 72 calls a width, each option with many counts
            kind, lvalid, rvalid, lbroad, rbroad = next(options)
            offs = next(offsets)
            lead = 0 if w in (16, 32) else w * int(rng.integers(0, 4))   # the output at several phases of its 16-byte line
            run_if_else(ctx, n, w, kind, offs, lvalid, rvalid, lbroad, rbroad, rng, lead=lead)


@pytest.mark.parametrize("w", (8, 3, 1))
def test_if_else_every_option(ctx, w):
    """the whole product of the options at one row count with a partial last step, byte and wave (B + 1 would do no more)"""
    rng = np.random.default_rng(100 + w)
    n = 3 * rows_per_wave(w) + 9
    offsets = itertools.cycle(itertools.product(OFFSETS, OFFSETS, OFFSETS))
    for kind, lvalid, rvalid, lbroad, rbroad in itertools.product(COND_KINDS, (True, False), (False, True), (False, True), (False, True)):
        run_if_else(ctx, n, w, kind, next(offsets), lvalid, rvalid, lbroad, rbroad, rng)
    run_if_else(ctx, n, w, "random", (3, 0, 69), True, False, True, False, rng, scalar_valid=False)   # a null scalar


@pytest.mark.parametrize("offs", list(itertools.product(OFFSETS, OFFSETS, OFFSETS)), ids=lambda o: "%d_%d_%d" % o)
def test_if_else_every_offset_triple(ctx, offs):
    rng = np.random.default_rng(sum(offs))
    for w in (8, 4, 16):
        run_if_else(ctx, rows_per_workgroup(w) + 1, w, "random_nulls", offs, True, True, False, False, rng)


@pytest.mark.parametrize("phase", range(16))
def test_if_else_output_phase_at_width_1(ctx, phase):
    rng = np.random.default_rng(phase)
    for n in (rows_per_workgroup(1) + 1, 65):
        run_if_else(ctx, n, 1, "random_nulls", (3, 69, 0), True, True, False, phase % 2 == 1, rng, lead=phase)


# ---- ah_if_else_boolean -------------------------------------------------------------------------------------------------------------
def test_if_else_boolean(ctx):
    rng = np.random.default_rng(7)
    b = K_BLOCK * 64   # a thread owns a 64-bit word
    options = itertools.cycle(itertools.product(COND_KINDS, (True, False), (False, True), (False, True), (False, True)))
    offsets = itertools.cycle(itertools.product(OFFSETS, OFFSETS, OFFSETS))
    for n in sizes(b):
        for _ in range(8):
            kind, lvalid, rvalid, lbroad, rbroad = next(options)
            offs = next(offsets)
            cond = Cond(ctx, kind, n, offs[0], rng)
            left = Side(ctx, "bool", n, offs[1], lvalid, lbroad, rng)
            right = Side(ctx, "bool", n, offs[2], rvalid, rbroad, rng)
            want_data, want_valid = CM.if_else_boolean(*cond.model(), left.model, right.model, n)
            od = guarded(ctx, (n + 7) // 8, "if_else_boolean data")
            ov = None if want_valid is None else guarded(ctx, (n + 7) // 8, "if_else_boolean validity")
            ctx.if_else_boolean(*cond.dev(), left.dev, right.dev, n, od, ov)
            ctx.sync()
            what = ("ah_if_else_boolean", n, kind, offs, lvalid, rvalid, lbroad, rbroad)
            od.check(str(what))
            check_bytes(od.download(np.uint8, (n + 7) // 8), want_data, what)
            if ov is not None:
                ov.check(str(what))
                check_bytes(ov.download(np.uint8, (n + 7) // 8), want_valid, what)


# ---- the var-length pair ------------------------------------------------------------------------------------------------------------------
LONG_ROW = 5000   # longer than a copy step of a whole workgroup (kBlock lanes x 4 bytes)


def row_lengths(n, rng):
    lens = np.array([0, 1, 15, 16, 17])[rng.integers(0, 5, max(n, 1))]
    lens[rng.integers(0, len(lens))] = LONG_ROW
    return lens


@pytest.mark.parametrize("widths", [(4, 4, 4), (4, 8, 8), (8, 4, 8), (8, 8, 4)], ids=lambda t: "l%d_r%d_out%d" % t)
def test_if_else_binary(ctx, widths):
    lw, rw, outw = widths
    assert LONG_ROW > K_BLOCK * 4
    rng = np.random.default_rng(sum(widths))
    options = itertools.cycle(itertools.product(COND_KINDS, (True, False), (False, True), (False, True), (False, True)))
    offsets = itertools.cycle(itertools.product(OFFSETS, OFFSETS, OFFSETS))
    for n in sizes(K_BLOCK):   # a row per lane, kBlock rows per workgroup step
        for _ in range(3):
            kind, lvalid, rvalid, lbroad, rbroad = next(options)
            offs = next(offsets)
            cond = Cond(ctx, kind, n, offs[0], rng)
            left = Side(ctx, "binary", n, offs[1], lvalid, lbroad, rng, ow=lw, lengths=row_lengths(n, rng))
            right = Side(ctx, "binary", n, offs[2], rvalid, rbroad, rng, ow=rw, lengths=row_lengths(n, rng))
            want_offsets, want_valid, want_total = CM.if_else_binary_offsets(*cond.model(), left.model, right.model, n, outw)
            oo = guarded(ctx, (n + 1) * outw, "if_else_binary offsets")
            ov = None if want_valid is None else guarded(ctx, (n + 7) // 8, "if_else_binary validity")
            what = ("ah_if_else_binary", n, widths, kind, offs, lvalid, rvalid, lbroad, rbroad)
            total = ctx.if_else_binary_offsets(*cond.dev(), left.dev, right.dev, n, outw, oo, ov)
            oo.check(str(what))
            assert total == want_total, what
            check_bytes(oo.download(want_offsets.dtype, n + 1), want_offsets, what)
            if ov is not None:
                ov.check(str(what))
                check_bytes(ov.download(np.uint8, (n + 7) // 8), want_valid, what)
            od = guarded(ctx, total, "if_else_binary data")
            ctx.if_else_binary_data(*cond.dev(), left.dev, right.dev, n, outw, oo, od)
            ctx.sync()
            od.check(str(what))
            oo.check(str(what))
            check_bytes(od.download(np.uint8, total), CM.if_else_binary_data(*cond.model(), left.model, right.model, n, want_offsets), what)


def test_if_else_binary_offset_overflow(ctx):
    """2^12 rows of one broadcast 2^20-byte row are 2^32 bytes: refused with 4-byte output offsets, counted with 8-byte ones.  Only the
    offsets call runs, and it reads no value byte: nothing of that size is allocated."""
    import arrow_go_amd as ah
    n = 1 << 12
    rng = np.random.default_rng(1)
    cond = Cond(ctx, "random", n, 3, rng)
    offsets = ctx.to_device(np.array([0, 1 << 20], np.int32), pad=8)
    dummy = ctx.to_device(np.zeros(16, np.uint8))
    side = (4, 0, offsets, dummy, None, 0, 1)
    m_side = (4, 0, np.array([0, 1 << 20], np.int32), None, None, 0, 1)
    oo = guarded(ctx, (n + 1) * 8, "offsets")
    with pytest.raises(CM.OffsetOverflow):
        CM.if_else_binary_offsets(*cond.model(), m_side, m_side, n, 4)
    with pytest.raises(ah.ErrInvalid, match="binary output offset overflow"):
        ctx.if_else_binary_offsets(*cond.dev(), side, side, n, 4, oo, None)
    oo.check("ah_if_else_binary_offsets, overflow")
    assert ctx.if_else_binary_offsets(*cond.dev(), side, side, n, 8, oo, None) == 1 << 32
    oo.check("ah_if_else_binary_offsets, 8-byte offsets")
    check_bytes(oo.download(np.int64, n + 1), np.arange(n + 1, dtype=np.int64) << 20, "offsets")


# ---- the directed fills ---------------------------------------------------------------------------------------------------------------------
FILL_SIZES = [0, 1, 63, 64, 65, S - 1, S, S + 1, 3 * S + 17]
LAYOUTS = ["all_valid", "no_bitmap", "all_null", "first_only", "last_only", "long_leading_run", "word_and_workgroup_ends", "nulls_10", "nulls_99"]


def layout_flags(layout, n, rng):
    """→ bools by row, or None for a call without a bitmap"""
    if layout == "no_bitmap":
        return None
    v = np.zeros(n, bool)
    if layout == "all_valid":
        v[:] = True
    elif layout == "first_only":
        v[:1] = True
    elif layout == "last_only":
        v[n - 1:] = True
    elif layout == "long_leading_run":   # S + 5 nulls (as many as fit), then every other row valid: forward leaves the run null,
        run = min(max(n - 1, 0), S + 5)  # backward fills it from a row of the next workgroup
        v[run::2] = True
    elif layout == "word_and_workgroup_ends":   # the last row of every 64-bit word — and so of every S rows
        v[63::64] = True
    elif layout == "nulls_10":
        v = rng.random(n) >= 0.10
    elif layout == "nulls_99":
        v = rng.random(n) >= 0.99
    return v


@pytest.fixture(scope="module")
def fill_values():
    """one column of the largest case's rows at the widest width, shared by every fill test and never changed"""
    return np.random.default_rng(5).integers(1, 256, (3 * S + 17 + max(OFFSETS)) * 32, dtype=np.uint8)


def run_fill(ctx, n, flags, off, direction, w, values, rng):
    """w = 0: ah_fill_null_indices, else ah_fill_null_directed of w-byte values"""
    valid = None if flags is None else bitmap_of(flags, off, rng)
    d_valid = None if valid is None else ctx.to_device(valid, pad=8)
    ov = None if valid is None else guarded(ctx, (n + 7) // 8, "fill validity")
    what = ("fill", n, off, direction, w)
    if w == 0:
        want, want_valid, want_nulls = CM.fill_null_indices(valid, off, n, direction)
        out = guarded(ctx, n * 4, "fill indices")
        nulls = ctx.fill_null_indices(d_valid, off, n, direction, out, ov)
    else:
        col = values[:(off + n) * w]
        want, want_valid, want_nulls = CM.fill_null_directed(w, col, valid, off, n, direction)
        d_values = ctx.to_device(col, pad=16)
        out = guarded(ctx, n * w, "fill values")
        nulls = ctx.fill_null_directed(w, d_values, d_valid, off, n, direction, out, ov)
    ctx.sync()
    out.check(str(what))
    assert nulls == want_nulls, what
    check_bytes(out.download(np.uint8, n * max(w, 4) if w == 0 else n * w), want, what)
    if ov is not None:
        ov.check(str(what))
        check_bytes(ov.download(np.uint8, (n + 7) // 8), want_valid, what)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", FILL_SIZES)
def test_fills(ctx, fill_values, n, layout):
    rng = np.random.default_rng(n + LAYOUTS.index(layout))
    flags = layout_flags(layout, n, rng)
    widths = itertools.cycle(VECTOR_WIDTHS)
    for direction in (0, 1):
        for off in OFFSETS if flags is not None else (0, 3):
            run_fill(ctx, n, flags, off, direction, 0, fill_values, rng)
            run_fill(ctx, n, flags, off, direction, next(widths), fill_values, rng)


@pytest.mark.parametrize("w", VECTOR_WIDTHS)
def test_fill_directed_every_width(ctx, fill_values, w):
    rng = np.random.default_rng(w)
    for n in (65, S + 1):
        for layout in ("nulls_10", "nulls_99", "long_leading_run"):
            for direction in (0, 1):
                run_fill(ctx, n, layout_flags(layout, n, rng), OFFSETS[(w + direction) % 3], direction, w, fill_values, rng)


def test_fill_without_the_null_count_does_not_need_it(ctx, fill_values):
    rng = np.random.default_rng(2)
    n, off = S + 1, 3
    flags = layout_flags("nulls_10", n, rng)
    valid = bitmap_of(flags, off, rng)
    col = fill_values[:(off + n) * 8]
    out, ov = guarded(ctx, n * 8, "fill values"), guarded(ctx, (n + 7) // 8, "fill validity")
    assert ctx.fill_null_directed(8, ctx.to_device(col, pad=16), ctx.to_device(valid, pad=8), off, n, 0, out, ov, want_null_count=False) is None
    ctx.sync()
    out.check("fill")
    ov.check("fill")
    want, want_valid, _ = CM.fill_null_directed(8, col, valid, off, n, 0)
    check_bytes(out.download(np.uint8, n * 8), want, "values")
    check_bytes(ov.download(np.uint8, (n + 7) // 8), want_valid, "validity")


# ---- edges of the interface ---------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_runs(ctx):
    import arrow_go_amd as ah
    out = guarded(ctx, 64, "untouched")
    bits = ctx.to_device(np.full(16, 0xFF, np.uint8))
    fixed8 = (0, 8, None, bits, None, 0, 0)
    calls = [
        (ah.ErrNotImplemented, lambda: ctx.fill_null_indices(bits, 0, 1 << 32, 0, out, out)),          # beyond 2^32 - 1 rows
        (ah.ErrNotImplemented, lambda: ctx.fill_null_directed(8, bits, bits, 0, 1 << 32, 1, out, out)),
        (ah.ErrNotImplemented, lambda: ctx.fill_null_directed(3, bits, bits, 0, 8, 0, out, out)),       # no fused route for 3-byte values
        (ah.ErrInvalid, lambda: ctx.fill_null_indices(bits, 0, 8, 2, out, out)),                        # no such direction
        (ah.ErrInvalid, lambda: ctx.fill_null_indices(bits, 0, 8, 0, out, None)),                       # a bitmap in, none out
        (ah.ErrInvalid, lambda: ctx.if_else(bits, None, 0, fixed8, (0, 4, None, bits, None, 0, 0), 8, out, None)),   # widths differ
        (ah.ErrInvalid, lambda: ctx.if_else(bits, bits, 0, fixed8, fixed8, 8, out, None)),              # a bitmap in, none out
        (ah.ErrInvalid, lambda: ctx.if_else(bits, None, 0, (4, 0, bits, bits, None, 0, 0), fixed8, 8, out, None)),   # a var-length side
        (ah.ErrInvalid, lambda: ctx.if_else(bits, None, -1, fixed8, fixed8, 8, out, None)),
        (ah.ErrInvalid, lambda: ctx.if_else_binary_offsets(bits, None, 0, fixed8, fixed8, 8, 4, out, None)),          # fixed sides
        (ah.ErrInvalid, lambda: ctx.if_else_binary_offsets(bits, None, 0, (4, 0, bits, bits, None, 0, 0), (8, 0, bits, bits, None, 0, 0), 8, 2, out, None)),
    ]
    for err, call in calls:
        with pytest.raises(err):
            call()
    ctx.sync()
    out.check("refused calls")
    assert out.download(np.uint8, 64).tolist() == [FILL] * 64


def test_no_rows_touch_nothing(ctx):
    out = guarded(ctx, 0, "empty")
    bits = ctx.to_device(np.zeros(8, np.uint8))
    side = (0, 8, None, bits, bits, 0, 0)
    ctx.if_else(bits, bits, 0, side, side, 0, out, out)
    ctx.if_else_boolean(bits, bits, 0, side, side, 0, out, out)
    assert ctx.fill_null_indices(bits, 0, 0, 0, out, out) == 0
    assert ctx.fill_null_directed(8, bits, bits, 0, 0, 1, out, out) == 0
    ctx.sync()
    out.check("n = 0")
