"""ah_window_flags / ah_window_rank / ah_window_scan through the C ABI against the host model (tests/window_model.py, itself
pinned in tests/test_window_model_host.py), every output in a GuardedBuffer whose two bands are read back after every call.

The rank and scan calls take the flags as an INPUT, so they are tested with flags laid out by hand — run lengths over the sorted
positions — and not with what ah_window_flags computes; that call has its own tests at the end.  With TILE and kSuper read from
ah_window.hip and S = kSuper * TILE (the rows of one workgroup of the sums pass):

  row counts   0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, S - 1, S, S + 1, 3 S + 17
  layouts      one partition (the carry crosses every tile and super tile); every row its own; runs of exactly TILE and of exactly S
               (the starts fall on the edges); a start at the last position of every tile and at the first of the next; one run
               longer than 2 S followed by runs of 1; random run lengths of mean 3 and mean 1000
  orders       the identity (NULL), a random permutation, the reverse

How the product is walked, so that no case takes more than about a second of host-model loops:
  test_ranks_and_count      every row count x every layout, all three orders inside: the three rank kinds and COUNT
  test_every_row_count      every row count, every layout inside with the orders, eight value types, the null rates and the offsets rotating:
                            SUM, MIN and MAX
  test_every_type           every layout x every one of the ten types at S + 1 rows (nine tiles, two super tiles), all three orders
                            inside: SUM, MIN and MAX with 0 %, 10 % and 100 % nulls, each at validity offsets 0, 3 and 69
Float columns hold integer values there (every prefix sum an integer below 2^53), so they too are compared byte for byte; general
float data has its own test with the bound every summation order in double meets."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import window_model as WM
from tests.backends import GuardedBuffer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "arrow_go_amd", "csrc", "ah_window.hip")).read()
TILE = int(re.search(r"constexpr int TILE = (\d+);", _SRC).group(1))
K_SUPER = int(re.search(r"constexpr int kSuper = (\d+);", _SRC).group(1))
S = K_SUPER * TILE
SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, S - 1, S, S + 1, 3 * S + 17]
LAYOUTS = ["one", "singles", "tile_runs", "super_runs", "tile_edges", "long_then_singles", "mean3", "mean1000"]
ORDERS = ["identity", "permutation", "reverse"]
ROW_NUMBER, RANK, DENSE_RANK = 0, 1, 2
SUM, MIN, MAX, COUNT = 0, 1, 2, 3
OPS = {SUM: "sum", MIN: "min", MAX: "max"}
TYPE_ID = {np.uint8: 2, np.int8: 3, np.uint16: 4, np.int16: 5, np.uint32: 6, np.int32: 7, np.uint64: 8, np.int64: 9, np.float32: 11, np.float64: 12}
DTYPES = list(TYPE_ID)
FILL = 0xCD   # what an output holds before the call: a row the kernel does not write shows


@pytest.fixture(scope="module")
def ctx():
    import arrow_go_amd as ah
    with ah.Context(0) as c:
        yield c


def run_lengths(layout, n, rng):
    if n == 0:
        return []
    if layout == "one":
        runs = [n]
    elif layout == "singles":
        runs = [1] * n
    elif layout in ("tile_runs", "super_runs"):
        step = TILE if layout == "tile_runs" else S
        runs = [step] * (n // step) + ([n % step] if n % step else [])
    elif layout == "tile_edges":   # starts at k TILE - 1 and at k TILE
        starts = sorted({0} | {p for k in range(1, n // TILE + 2) for p in (k * TILE - 1, k * TILE) if 0 < p < n})
        runs = [b - a for a, b in zip(starts, starts[1:] + [n])]
    elif layout == "long_then_singles":
        first = min(n, 2 * S + 5)
        runs = [first] + [1] * (n - first)
    else:
        mean = 3 if layout == "mean3" else 1000
        runs, left = [], n
        while left:
            r = min(left, int(rng.geometric(1.0 / mean)))
            runs.append(r)
            left -= r
    assert sum(runs) == n
    return runs


def flags_of(runs, n, rng):
    """bit 0 at every run's first position; bit 1 there and at about a third of the other positions"""
    fl = (rng.random(n) < 0.35).astype(np.uint8) * 2
    p = 0
    for r in runs:
        fl[p] = 3
        p += r
    return fl


def order_of(kind, n, rng):
    if kind == "identity":
        return None
    return (rng.permutation(n) if kind == "permutation" else np.arange(n - 1, -1, -1)).astype(np.uint64)


class Case:
    """flags and order of one (n, layout, order kind) on the device and as the model's lists"""

    def __init__(self, ctx, n, layout, order_kind, seed):
        rng = np.random.default_rng(seed)
        self.ctx, self.n = ctx, n
        self.flags = flags_of(run_lengths(layout, n, rng), n, rng)
        self.order = order_of(order_kind, n, rng)
        self.d_flags = ctx.to_device(self.flags, pad=8)
        self.d_order = None if self.order is None else ctx.to_device(self.order, pad=8)
        self.m_flags = self.flags.tolist()
        self.m_order = list(range(n)) if self.order is None else self.order.tolist()

    def rank(self, kind):
        out = GuardedBuffer(self.ctx, self.n * 8, name="ranks")
        out.memset(FILL)
        self.ctx.window_rank(kind, self.d_flags, self.d_order, self.n, out)
        self.ctx.sync()
        out.check("ah_window_rank kind %d" % kind)
        return out.download(np.uint64, self.n)

    def scan(self, op, values, valid, voff=0, out_dtype=None):
        """values: numpy by row; valid: bools by row or None (no bitmap)"""
        dt = values.dtype
        out_dtype = out_dtype or (dt if op in (MIN, MAX) else np.int64 if op == COUNT else {"i": np.int64, "u": np.uint64, "f": np.float64}[dt.kind])
        out = GuardedBuffer(self.ctx, self.n * np.dtype(out_dtype).itemsize, name="window values")
        out.memset(FILL)
        d_vals = self.ctx.to_device(values, pad=8)
        d_valid = None
        if valid is not None:
            bits = np.concatenate([np.random.default_rng(voff).random(voff) < 0.5, valid]).astype(np.uint8)
            d_valid = self.ctx.to_device(np.packbits(bits, bitorder="little"), pad=8)
        self.ctx.window_scan(op, TYPE_ID[dt.type], d_vals, d_valid, voff, self.d_flags, self.d_order, self.n, out)
        self.ctx.sync()
        out.check("ah_window_scan op %d %s" % (op, dt))
        return out.download(out_dtype, self.n)


def values_of(dt, n, rng):
    """integers of the type's whole range for the narrow types, such that 64-bit sums wrap for the wide ones; floats hold integers
    whose prefix sums stay below 2^53"""
    dt = np.dtype(dt)
    if dt.kind == "f":
        return rng.integers(-1000, 1000, n).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def nulls_of(rate, n, rng):
    return None if rate == 0 else (rng.random(n) >= 0.1 if rate == 10 else np.zeros(n, bool))


def expect(op, values, valid, case):
    want = WM.running(OPS[op], values, valid, case.m_flags, case.m_order)
    if isinstance(want, list):   # exact fractions of integer-valued floats
        want = np.array([float(f) for f in want], np.float64)
    return want


# ---- ranks and counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
def test_ranks_and_count(ctx, n, layout):
    for oi, order_kind in enumerate(ORDERS):
        case = Case(ctx, n, layout, order_kind, seed=n * 31 + oi)
        want = WM.ranks(case.m_flags, case.m_order)
        for kind in (ROW_NUMBER, RANK, DENSE_RANK):
            assert case.rank(kind).tobytes() == want[kind].tobytes(), (n, layout, order_kind, kind)
        rng = np.random.default_rng(n + 7)
        valid = nulls_of(10, n, rng)
        got = case.scan(COUNT, np.zeros(n, np.int32), valid, voff=3)
        assert got.tobytes() == WM.running("count", None, valid, case.m_flags, case.m_order).tobytes(), (n, layout, order_kind)
    if n:   # without a bitmap the count is the row number
        assert case.scan(COUNT, np.zeros(n, np.int8), None).tobytes() == want[ROW_NUMBER].astype(np.int64).tobytes()


@pytest.mark.parametrize("n", SIZES)
def test_every_row_count(ctx, n):
    rng = np.random.default_rng(n)
    for li, layout in enumerate(LAYOUTS):
        case = Case(ctx, n, layout, ORDERS[(li + n) % 3], seed=n * 17 + li)
        dt = (np.int64, np.float64, np.int8, np.uint32, np.float32, np.uint64, np.int16, np.uint8)[li]
        values, valid = values_of(dt, n, rng), nulls_of((10, 0, 100)[(li + n) % 3], n, rng)
        for op in OPS:
            got = case.scan(op, values, valid, voff=(0, 3, 69)[li % 3])
            assert got.tobytes() == expect(op, values, valid, case).tobytes(), (n, layout, np.dtype(dt).name, OPS[op])


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_type(ctx, layout, dt):
    n = S + 1
    rng = np.random.default_rng(LAYOUTS.index(layout) * 100 + DTYPES.index(dt))
    values = values_of(dt, n, rng)
    for oi, order_kind in enumerate(ORDERS):
        case = Case(ctx, n, layout, order_kind, seed=oi + 3)
        for rate in (0, 10, 100):
            valid = nulls_of(rate, n, rng)
            for op in OPS:
                want = expect(op, values, valid, case).tobytes()
                for voff in (0, 3, 69):
                    if valid is None and voff:
                        continue   # no bitmap, no offset
                    assert case.scan(op, values, valid, voff).tobytes() == want, (layout, np.dtype(dt).name, order_kind, rate, OPS[op], voff)
            if rate == 0:   # a bitmap of ones is the same as none
                assert case.scan(SUM, values, np.ones(n, bool), 69).tobytes() == expect(SUM, values, None, case).tobytes()


# ---- floats ---------------------------------------------------------------------------------------------------------------------------
U = Fraction(1, 2**53)


@pytest.mark.parametrize("data", ["normal", "forty_binades"])
@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float32", "float64"])
def test_float_sums_meet_the_bound_of_every_summation_order(ctx, dt, data):
    """|got - exact| <= gamma(c - 1) * sum |x| over the c valid addends of the prefix, gamma(m) = m u / (1 - m u), u = 2^-53: the
    bound of recursive summation in any order (Higham, Accuracy and Stability of Numerical Algorithms, §4.2), so it is derived and
    not measured.  A second call returns the same bytes."""
    n = S + 1
    rng = np.random.default_rng(11)
    values = rng.standard_normal(n) if data == "normal" else rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))
    values = values.astype(dt)
    for layout, order_kind, rate in (("one", "permutation", 10), ("mean1000", "identity", 0), ("mean3", "reverse", 10), ("tile_edges", "permutation", 0)):
        case = Case(ctx, n, layout, order_kind, seed=5)
        valid = nulls_of(rate, n, rng)
        got = case.scan(SUM, values, valid, voff=3 if valid is not None else 0)
        assert got.tobytes() == case.scan(SUM, values, valid, voff=3 if valid is not None else 0).tobytes(), "a second call gave other bytes"
        exact = WM.running("sum", values, valid, case.m_flags, case.m_order)
        c, mag = 0, Fraction(0)
        for p, r in enumerate(case.m_order):
            if case.m_flags[p] & 1:
                c, mag = 0, Fraction(0)
            if valid is not None and not valid[r]:
                assert got[r] == 0 and not np.signbit(got[r])
                continue
            c += 1
            mag += abs(Fraction(float(values[r])))
            m = (c - 1) * U
            assert abs(Fraction(float(got[r])) - exact[r]) <= m / (1 - m) * mag, (layout, order_kind, p, r, c)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float32", "float64"])
def test_float_min_max_nan_and_zero_rules(ctx, dt):
    """NaNs are ignored unless every valid value so far is one (then the canonical quiet NaN, whatever payload came in); -0 < +0"""
    n = TILE + 1
    rng = np.random.default_rng(3)
    nan2 = np.array([0xFFF8000000000123], np.uint64).view(np.float64)[0] if dt == np.float64 else np.array([0xFFC00123], np.uint32).view(np.float32)[0]
    pool = np.array([np.nan, nan2, -0.0, 0.0, 1.5, -1.5, np.inf, -np.inf, 3.0], dt)
    for layout, order_kind in (("mean3", "permutation"), ("one", "identity"), ("mean1000", "reverse")):
        case = Case(ctx, n, layout, order_kind, seed=9)
        values = pool[rng.integers(0, len(pool), n)]
        first = case.m_order[:40]
        values[first] = pool[rng.integers(0, 2, len(first))]   # the column opens with NaNs only …
        values[case.m_order[40:60]] = pool[rng.integers(2, 4, 20)]   # … then zeros of both signs
        for valid in (None, nulls_of(10, n, rng)):
            for op in (MIN, MAX):
                got = case.scan(op, values, valid, voff=69 if valid is not None else 0)
                assert got.tobytes() == expect(op, values, valid, case).tobytes(), (layout, order_kind, OPS[op], valid is None)


# ---- edges of the interface ------------------------------------------------------------------------------------------------------------
def test_too_many_rows_and_bad_arguments_are_refused_before_anything_runs(ctx):
    import arrow_go_amd as ah
    out = GuardedBuffer(ctx, 64, name="untouched")
    out.memset(FILL)
    flags = ctx.to_device(np.full(8, 3, np.uint8))
    for call in (lambda: ctx.window_rank(RANK, flags, None, (1 << 30) + 1, out),
                 lambda: ctx.window_scan(SUM, 9, flags, None, 0, flags, None, (1 << 30) + 1, out),
                 lambda: ctx.window_flags(None, [], None, (1 << 30) + 1, out),
                 lambda: ctx.window_rank(7, flags, None, 8, out),
                 lambda: ctx.window_scan(9, 9, flags, None, 0, flags, None, 8, out),
                 lambda: ctx.window_scan(SUM, 14, flags, None, 0, flags, None, 8, out),
                 lambda: ctx.window_rank(RANK, flags, None, -1, out)):
        with pytest.raises(ah.ArrowHipError):
            call()
    ctx.sync()
    out.check("refused calls")
    assert out.download(np.uint8, 64).tolist() == [FILL] * 64


# ---- ah_window_flags ------------------------------------------------------------------------------------------------------------------
def _bitmap(ctx, valid, off):
    bits = np.concatenate([np.zeros(off, bool), valid]).astype(np.uint8)
    return ctx.to_device(np.packbits(bits, bitorder="little"), pad=8)


def _numeric_key(ctx, values, valid, off):
    """(ah_sort_key tuple, the model's list): row i is element off + i"""
    buf = ctx.to_device(np.concatenate([np.zeros(off, values.dtype), values]), pad=8)
    vb = None if valid is None else _bitmap(ctx, valid, off)
    pl = [None if valid is not None and not valid[i] else v for i, v in enumerate(values.tolist())]
    return (TYPE_ID[values.dtype.type], buf, None, 0, vb, off, 0, 0), pl, (buf, vb)


def _string_key(ctx, strings, off):
    raw = [b"junk"] * off + [b"" if s is None else s for s in strings]
    offsets = np.zeros(len(raw) + 1, np.int32)
    offsets[1:] = np.cumsum([len(b) for b in raw])
    data = np.frombuffer(b"".join(raw) or b"\0", np.uint8)
    valid = np.array([s is not None for s in strings])
    bufs = (ctx.to_device(offsets, pad=8), ctx.to_device(data, pad=8), _bitmap(ctx, valid, off))
    return (14, bufs[1], bufs[0], 0, bufs[2], off, 0, 0), list(strings), bufs


def _decimal_key(ctx, ints, off):
    raw = b"".join((0 if v is None else v).to_bytes(16, "little", signed=True) for v in [0] * off + list(ints))
    valid = np.array([v is not None for v in ints])
    bufs = (ctx.to_device(np.frombuffer(raw, np.uint8), pad=8), _bitmap(ctx, valid, off))
    return (23, bufs[0], None, 16, bufs[1], off, 0, 0), list(ints), bufs


def _keys(ctx, kind, n, rng):
    """→ [(key tuple, model list, buffers)]"""
    if kind == "int64":
        return [_numeric_key(ctx, rng.integers(-2, 3, n).astype(np.int64) * (1 << 40), rng.random(n) < 0.8, 3)]
    if kind == "float64":
        pool = np.array([np.nan, np.array([0x7FF8000000000001], np.uint64).view(np.float64)[0], -0.0, 0.0, 1.0, -1.0], np.float64)
        return [_numeric_key(ctx, pool[rng.integers(0, len(pool), n)], rng.random(n) < 0.8, 69)]
    if kind == "float32":
        return [_numeric_key(ctx, np.array([np.nan, -0.0, 0.0, 2.5], np.float32)[rng.integers(0, 4, n)], None, 0)]
    if kind == "int8":
        return [_numeric_key(ctx, rng.integers(-1, 2, n).astype(np.int8), rng.random(n) < 0.9, 5)]
    if kind == "string":   # a proper-prefix pair, an empty value, values longer than a word, a null
        pool = [b"ab", b"abc", b"", None, b"0123456789abcdef-x", b"0123456789abcdef-y", b"ab\0"]
        return [_string_key(ctx, [pool[i] for i in rng.integers(0, len(pool), n)], 3)]
    if kind == "decimal128":
        pool = [0, 1, -1, None, 1 << 64, -(1 << 64), (1 << 64) + 1, 10**30]
        return [_decimal_key(ctx, [pool[i] for i in rng.integers(0, len(pool), n)], 2)]
    assert kind == "two_keys"
    return _keys(ctx, "int8", n, rng) + _keys(ctx, "string", n, rng)


@pytest.mark.parametrize("with_parts", [False, True], ids=["one_partition", "part_ids"])
@pytest.mark.parametrize("kind", ["int64", "float64", "float32", "int8", "string", "decimal128", "two_keys", "no_keys"])
def test_flags(ctx, kind, with_parts):
    n = TILE + 1
    rng = np.random.default_rng(len(kind) + with_parts)
    keys = [] if kind == "no_keys" else _keys(ctx, kind, n, rng)
    pids = rng.integers(0, 3, n).astype(np.int32) if with_parts else None
    d_pids = None if pids is None else ctx.to_device(pids, pad=8)
    for order in (None, rng.permutation(n).astype(np.uint64)):
        m_order = list(range(n)) if order is None else order.tolist()
        d_order = None if order is None else ctx.to_device(order, pad=8)
        out = GuardedBuffer(ctx, n, name="flags")
        out.memset(FILL)
        ctx.window_flags(d_pids, [k[0] for k in keys], d_order, n, out)
        ctx.sync()
        out.check("ah_window_flags " + kind)
        want = WM.flags(None if pids is None else pids.tolist(), [k[1] for k in keys], m_order)
        assert out.download(np.uint8, n).tolist() == want, (kind, with_parts, order is None)
        assert len(set(want)) > 1 or kind == "no_keys"   # the data does tie and does differ


def test_flags_of_no_rows_touch_nothing(ctx):
    out = GuardedBuffer(ctx, 0, name="flags")
    ctx.window_flags(None, [], None, 0, out)
    ctx.sync()
    out.check("ah_window_flags n = 0")
