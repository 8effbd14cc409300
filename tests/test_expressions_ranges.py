"""Both routes of eval_expression — one JIT-compiled kernel (fuse=True) and one kernel per call node (fuse=False) — against the
independent model of tests/expr_model.py, over full value ranges.

The two routes compile the same ah_elementwise.h, so a mistake in that text passes a test that only compares them.  What the fused
route has of its own is what these cases aim at: the generated skeleton (the wave-uniform chunk loop with its inactive unrolled
steps, load_bits64 across two words, store_word, the ballots), the slot rule of the checked ops as Generate() restates it, the
AH_X_CAST nodes, literals passed as 8-byte kernel arguments, and hiprtc's option list (contraction off, IEEE denormals).

Every case compares each route with the model on four points: result type, value bytes (the payload under nulls included; NaN
payloads excepted), validity bits (an absent bitmap == all valid), and the error: the model's status "overflow" must come back as
ErrInvalid with "overflow" in its text, its "ok" as no error.

Shapes.  One workgroup of the fused kernel covers 4 waves × 4 chunks × 64 rows = 1024 rows, so the row counts are 1, 63, 64, 65,
1023, 1024, 1025 and 2 × 1024 + 77.  Every column is a slice with its own offset out of {0, 1, 7, 63, 64, 65}: the two-word branch
of load_bits64 runs for some columns of a call and not for others.  One column of a call has no nulls.
"""
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pytest

from tests import expr_model as M
from tests.test_gpu_parity import rand, same_bits_or_both_nan

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 77]
OFFSETS = [0, 1, 7, 63, 64, 65]
ALL_TYPES = ["uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64", "float32", "float64"]
INT_TYPES = ALL_TYPES[:8]


@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.close()


# ---- columns, literals, results ------------------------------------------------------------------------------
def arrow_type(dt):
    dt = np.dtype(dt)
    return pa.bool_() if dt == bool else pa.from_numpy_dtype(dt)


class Col:
    """a column as the model sees it (values of every slot, valid or None) and as the library gets it: a slice at `offset` of
    buffers whose leading rows hold other values and other validity bits"""

    def __init__(self, values, valid=None, offset=0, seed=0):
        rng = np.random.default_rng(1000 + seed + offset)
        self.values, self.valid = np.ascontiguousarray(values), valid
        n, dt = len(values), self.values.dtype
        if dt == bool:
            data = np.packbits(np.concatenate([rng.random(offset) < 0.5, self.values]), bitorder="little")
        else:
            lead = np.frombuffer(rng.bytes(offset * dt.itemsize), dt)
            data = np.concatenate([lead, self.values])
        vbuf, nulls = None, 0
        if valid is not None:
            bits = np.concatenate([rng.random(offset) < 0.5, valid])
            vbuf = pa.py_buffer(np.packbits(bits, bitorder="little").tobytes())
            nulls = int(n - np.count_nonzero(valid))
        self.arrow = pa.Array.from_buffers(arrow_type(dt), n, [vbuf, pa.py_buffer(data.tobytes())], null_count=nulls, offset=offset)

    def model(self):
        return self.values, self.valid


def literal(dtype, value):
    """→ (the model's literal, the library's)"""
    dt = np.dtype(dtype)
    py = None if value is None else (np.array([value], dt)[0].item())
    return (dt, None if value is None else np.array([value], dt)[0]), pa.scalar(py, type=arrow_type(dt))


def parts(arr):
    """(values of every slot, validity) of a result, restricted to its logical range"""
    n, off = len(arr), arr.offset
    bufs = arr.buffers()
    valid = np.ones(n, bool) if bufs[0] is None else np.unpackbits(np.frombuffer(bufs[0], np.uint8), bitorder="little")[off:off + n].astype(bool)
    if arr.type == pa.bool_():
        return np.unpackbits(np.frombuffer(bufs[1], np.uint8), bitorder="little")[off:off + n].astype(bool), valid
    dt = np.dtype(arr.type.to_pandas_dtype())
    return np.frombuffer(bufs[1], np.uint8)[off * dt.itemsize:(off + n) * dt.itemsize].view(dt), valid


def check(sess, text, cols, lits=(), what=None, model_values=True):
    """both routes against the model; returns the model's (values, validity, status)"""
    from arrow_go_amd import compute as ac
    lits = [literal(*l) for l in lits]
    mv, mk, status = M.evaluate(text, [c.model() for c in cols], [l[0] for l in lits])
    got = {}
    for fuse in (True, False):
        route = "fused" if fuse else "per call"
        try:
            out, was_fused = sess.eval_expression(text, [c.arrow for c in cols], [l[1] for l in lits], fuse=fuse)
        except ac.ArrowError as e:
            assert status == "overflow", (text, what, route, "the model reports no error, the route:", str(e))
            assert isinstance(e, ac.ErrInvalid) and "overflow" in str(e), (text, what, route, str(e))
            continue
        assert status == "ok", (text, what, route, "the model reports overflow, the route none")
        assert was_fused == fuse, (text, what, route)
        assert out.type == arrow_type(mv.dtype) and len(out) == len(mv), (text, what, route, out.type)
        v, k = parts(out)
        got[fuse] = (v, k)
        assert (k == mk).all(), (text, what, route, "validity", np.flatnonzero(k != mk)[:8])
        if model_values:
            same = (v == mv).all() if mv.dtype == bool else same_bits_or_both_nan(v, mv)
            assert same, (text, what, route, "values", [(i, v[i], mv[i]) for i in np.flatnonzero(v != mv)[:8]])
    if len(got) == 2:   # whatever the model leaves open, the routes agree on
        assert (got[True][0] == got[False][0]).all() if mv.dtype == bool else same_bits_or_both_nan(got[True][0], got[False][0]), (text, what, "fused vs per call")
    return mv, mk, status


def planted(rng, dtype, n, turn=0):
    """full-range random values (rand() of test_gpu_parity) with the type's boundary set planted at the first row, the last row,
    lane 63 of a chunk and lane 0 of the next (rows 63 | 64 and 1023 | 1024), and once as a whole from row 1 on; `turn` rotates
    the set, so that the columns of a call meet in different pairs"""
    a = rand(rng, dtype, n)
    b = np.roll(M.boundary(dtype), turn)
    if n >= 128:
        a[1:1 + len(b)] = b
    for j, row in enumerate([0, n - 1, 63, 64, 1023, 1024]):
        if row < n:
            a[row] = b[(j * 3) % len(b)]
    return a


def columns(dtype, n, turn, k=3):
    """k sliced columns of n rows: the second has no nulls, the others 20 % and 50 %"""
    rng = np.random.default_rng(n * 31 + turn)
    out = []
    for i in range(k):
        off = OFFSETS[(turn + (0, 1, 3)[i % 3]) % len(OFFSETS)]
        valid = None if i == 1 else rng.random(n) >= (0.2, 0, 0.5)[i % 3]
        out.append(Col(planted(rng, dtype, n, turn + 2 * i), valid, off, seed=i))
    return out


# ---- the trees of test_expressions.py, full range -----------------------------------------------------------------------
EXPRS = [
    ("greater(multiply_unchecked(add_unchecked($0,$1),$2),#0)", 3, [5]),
    ("and(greater($0,#0),less_equal($1,$2))", 3, [0]),
    ("subtract_unchecked(multiply_unchecked($0,$0),multiply_unchecked($1,#0))", 2, [3]),
    ("xor(equal($0,$1),invert(not_equal($2,#0)))", 3, [1]),
    ("add(abs_unchecked($0),sign($1))", 2, []),
    ("or(and_not(greater_equal($0,$1),less($1,$2)),equal($2,#0))", 3, [2]),
    ("multiply(add($0,$1),subtract($2,#0))", 3, [0]),
]


@pytest.mark.parametrize("tree", range(len(EXPRS)), ids=lambda i: f"tree{i}")
@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_trees_full_range(sess, dtype, tree):
    """the seven trees over full-range columns with the boundary values planted.  The two trees with checked ops mostly end in
    "overflow" here — the model says when; test_checked_boundaries has the arrays that overflow nowhere"""
    text, ncols, lits = EXPRS[tree]
    has_checked = "add(" in text or "multiply(" in text
    for turn, n in enumerate(ROWS):
        cols = columns(dtype, n, turn)[:ncols]
        _, _, status = check(sess, text, cols, [(dtype, v) for v in lits], (dtype, n))
        assert has_checked or status == "ok"
        if has_checked:   # … and the same tree over small operands, where it must succeed
            small = [Col((c.values.view(f"u{c.values.dtype.itemsize}") % 6).astype(dtype), c.valid, c.arrow.offset, seed=7) for c in cols]
            _, _, status = check(sess, text, small, [(dtype, v) for v in lits], (dtype, n, "small"))
            assert status == "ok"


@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_unary_full_range(sess, dtype):
    for turn, n in enumerate(ROWS):
        cols = columns(dtype, n, turn, k=1)
        for name in ("sign", "abs_unchecked", "negate_unchecked"):
            mv, _, status = check(sess, f"{name}($0)", cols, (), (dtype, n))
            assert status == "ok" and mv.dtype == np.dtype(dtype)   # every op keeps its operand's type


@pytest.mark.parametrize("name", M.COMPARE)
@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_comparisons_literal_on_each_side(sess, dtype, name):
    """the literal runs through the boundary set (a kernel argument: no new compile), on the right and on the left"""
    b = M.boundary(dtype)
    seen = set()
    for turn, n in enumerate(ROWS):
        cols = columns(dtype, n, turn, k=1)
        for j in range(3):
            lit = b[(turn * 3 + j) % len(b)]
            for text in (f"{name}($0,#0)", f"{name}(#0,$0)"):
                mv, _, _ = check(sess, text, cols, [(dtype, lit)], (dtype, n, lit))
                seen.update(mv.tolist())
    assert seen == {True, False}


def test_boolean_columns(sess):
    """Boolean INPUT columns: their data bits come through load_bits64 like the validity bits, each at its own offset"""
    for turn, n in enumerate(ROWS):
        rng = np.random.default_rng(50 + n)
        cols = []
        for i in range(3):
            valid = None if i == 1 else rng.random(n) >= 0.3
            cols.append(Col(rng.random(n) < 0.5, valid, OFFSETS[(turn + (0, 1, 3)[i]) % 6], seed=20 + i))
        num = columns("int32", n, turn, k=1)[0]
        for text in ("and_not($0,$1)", "xor(or($0,$1),invert($2))", "invert($0)"):
            check(sess, text, cols, (), n)
        check(sess, "and($0,or($2,greater($3,#0)))", cols + [num], [("int32", -1)], n)


# ---- implicit promotion at the narrow type's extremes -----------------------------------------------------------------------
def test_promotion_at_extremes(sess):
    for turn, n in enumerate(ROWS):
        rng = np.random.default_rng(60 + n)
        off = lambda i: OFFSETS[(turn + (0, 1, 3)[i]) % 6]   # noqa: E731
        mask = lambda p: rng.random(n) >= p                   # noqa: E731
        i8 = Col(planted(rng, "int8", n, turn), mask(0.2), off(0), seed=1)
        i16 = Col(planted(rng, "int16", n, turn), mask(0.2), off(0), seed=2)
        i32 = Col(planted(rng, "int32", n, turn), None, off(1), seed=3)
        u32 = Col(planted(rng, "uint32", n, turn), mask(0.2), off(0), seed=4)
        # wide partners that keep the checked sums in range: |x| < 2^62; the last row lands exactly on Int64's minimum
        w = rng.integers(-2**62, 2**62, n, dtype=np.int64)
        w[n - 1] = np.iinfo(np.int64).min - int(i8.values[n - 1]) if i8.values[n - 1] <= 0 else w[n - 1]
        i64 = Col(w, mask(0.5), off(2), seed=5)
        u64 = Col(planted(rng, "uint64", n, turn + 1), None, off(2), seed=6)
        f64 = Col(planted(rng, "float64", n, turn), mask(0.5), off(2), seed=7)
        f32 = Col(planted(rng, "float32", n, turn), None, off(1), seed=8)
        cases = [("add($0,$1)", [i8, i64], []),                        # int8 = −128 into Int64
                 ("multiply_unchecked($0,$1)", [u32, u64], []),        # uint32 = max into UInt64
                 ("greater($0,$1)", [i32, f64], []),                   # int32 = min into Float64
                 ("add($0,$1)", [i32, f64], []),
                 ("subtract($0,$1)", [i16, f32], []),                  # int16 into Float32
                 ("less($0,#0)", [i32], [("int64", 12345678901)]),     # a scalar is cast on the host, the column in the kernel
                 ("greater_equal(#0,$0)", [i8], [("int64", -128)])]
        for text, cols, lits in cases:
            mv, _, status = check(sess, text, cols, lits, n)
            assert status == "ok"
        if n >= 128:
            assert (i8.values == -128).any() and (u32.values == 2**32 - 1).any() and (i32.values == -2**31).any() and (i16.values == 2**15 - 1).any()


# ---- floats ---------------------------------------------------------------------------------------------------
def test_float32_denormals(sess):
    """denormal operands, and products and sums that land in the denormal range: the hiprtc build and the library build must both
    keep them (no flush to zero), as IEEE and the host model do"""
    n = ROWS[-1]
    rng = np.random.default_rng(70)
    tiny = np.finfo(np.float32).tiny
    den = rng.integers(1, 2**23, n).astype(np.uint32).view(np.float32) * rng.choice(np.array([1, -1], np.float32), n)   # denormal operands
    scale = rng.uniform(0.25, 2, n).astype(np.float32)
    small_a = (rng.uniform(1, 2, n) * 2.0**-80).astype(np.float32)      # normal × normal → denormal
    small_b = (rng.uniform(1, 2, n) * 2.0**-60).astype(np.float32)
    near = (rng.uniform(1, 2, n) * tiny).astype(np.float32)             # normal − normal → denormal
    near2 = (near * np.float32(1 + 2.0**-10)).astype(np.float32)
    cases = [("multiply_unchecked($0,$1)", [den, scale]), ("multiply_unchecked($0,$1)", [small_a, small_b]), ("add_unchecked($0,$1)", [den, den[::-1].copy()]),
             ("subtract_unchecked($0,$1)", [near2, near]), ("multiply($0,$1)", [den, scale]), ("subtract($0,$1)", [near2, near])]
    for i, (text, (a, b)) in enumerate(cases):
        cols = [Col(a, rng.random(n) >= 0.2, 7, seed=i), Col(b, None, 64, seed=i)]
        mv, _, _ = check(sess, text, cols, (), i)
        assert ((mv != 0) & (np.abs(mv) < tiny)).mean() > 0.5, (text, "the inputs must make most results denormal")
    mv, _, _ = check(sess, "multiply_unchecked($0,#0)", [Col(den, None, 1)], [("float32", 0.5)], "literal")
    assert ((mv != 0) & (np.abs(mv) < tiny)).mean() > 0.5


def nearest(fr, dtype):
    """the exact rational `fr` rounded to nearest-even in `dtype`"""
    with np.errstate(all="ignore"):
        x = np.array([float(fr)]).astype(dtype)[0]
    cands = [x, np.nextafter(x, dtype(np.inf)), np.nextafter(x, dtype(-np.inf))]
    u = f"u{np.dtype(dtype).itemsize}"
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - fr), int(np.array([c]).view(u)[0]) & 1))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_no_contraction(sess, dtype):
    """add(multiply($0,$1),$2) where a fused multiply-add would show: c = −fl(a·b) + k·ulp, so the twice-rounded result is k·ulp
    exactly, the contracted one k·ulp plus the product's rounding error.  The exact a·b + c (fractions.Fraction), rounded once, is
    what contraction would give; at least a tenth of the rows must tell it from the model's twice-rounded value"""
    n = ROWS[-1]
    rng = np.random.default_rng(80)
    a, b = rng.uniform(1, 2, n).astype(dtype), rng.uniform(1, 2, n).astype(dtype)
    p = a * b
    c = (-p + rng.integers(-4, 5, n).astype(dtype) * np.spacing(p)).astype(dtype)
    cols = [Col(a, rng.random(n) >= 0.2, 63, seed=1), Col(b, None, 1, seed=2), Col(c, rng.random(n) >= 0.2, 64, seed=3)]
    mv, _, status = check(sess, "add(multiply($0,$1),$2)", cols, (), np.dtype(dtype))
    contracted = np.array([nearest(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z)), dtype) for x, y, z in zip(a, b, c)], dtype)
    share = float((contracted != mv).mean())
    print(f"rows that tell a contracted result from the twice-rounded one: {share:.3f}")
    assert status == "ok" and share >= 0.1
    check(sess, "subtract_unchecked(multiply_unchecked($0,$1),$2)", [cols[0], cols[1], Col(-c, cols[2].valid, 64, seed=3)], (), np.dtype(dtype))


# ---- checked ops: arrays that overflow nowhere, then one slot at a time ----------------------------------------------------
def in_range_pairs(rng, dt, op, n):
    """n pairs (a, b) whose exact result under op lies in the type, drawn so that the results spread over the whole range"""
    lo, hi = M.limits(dt)
    ceil_div = lambda p, q: -((-p) // q)   # noqa: E731
    a, b = [], []
    for _ in range(n):
        if op == "multiply":    # a small factor, the other drawn from all of [lo / x, hi / x]
            x = int(rng.integers(1, 12)) * (1 if lo == 0 or rng.random() < 0.5 else -1)
            y_lo, y_hi = (ceil_div(lo, x), hi // x) if x > 0 else (ceil_div(hi, x), lo // x)
            y_lo, y_hi = max(lo, y_lo), min(hi, y_hi)
            y = y_lo + int(rng.integers(0, y_hi - y_lo, endpoint=True, dtype=np.uint64))
        else:                   # the result r drawn from the whole type, then a split of it
            r = int(rng.integers(lo, hi, endpoint=True, dtype=dt))
            x_lo, x_hi = (max(lo, r - hi), min(hi, r - lo)) if op == "add" else (max(lo, lo + r), min(hi, hi + r))
            x = int(rng.integers(x_lo, x_hi, endpoint=True, dtype=dt))
            y = r - x if op == "add" else x - r
        a.append(x)
        b.append(y)
    return np.array(a, dt), np.array(b, dt)


def boundary_pairs(dt, op):
    """→ (pairs whose result is exactly max, pairs whose result is exactly min, the first pair past max or None, the first pair
    below min or None: None where the type cannot get there)"""
    lo, hi = M.limits(dt)
    k, signed = 5, lo < 0
    if op == "add":
        up, down = [(hi - k, k), (hi, 0)], ([(lo + k, -k), (lo, 0)] if signed else [(0, 0)])
        return up, down, (hi - k, k + 1), ((lo + k, -k - 1) if signed else None)
    if op == "subtract":
        up = [(hi - k, -k), (hi, 0)] if signed else [(hi, 0)]
        down = [(lo + k, k), (lo, 0)] if signed else [(k, k), (0, 0)]
        return up, down, ((hi - k, -k - 1) if signed else None), (lo + k, k + 1)
    d = next(f for f in (3, 5, 7, 1) if hi % f == 0)   # a divisor of max (the maxima of Int8 and Int32 are prime: 1)
    up = [(hi // d, d), (hi, 1), (1, hi)] + ([(-hi, -1)] if signed else [])
    down = [(lo // 2, 2), (lo, 1), (1, lo)] if signed else [(0, hi), (hi, 0)]
    return up, down, (hi // d, d + 1), ((lo // 2 - 1, 2) if signed else None)


@pytest.mark.parametrize("op", ["add", "subtract", "multiply"])
@pytest.mark.parametrize("dtype", INT_TYPES)
def test_checked_boundaries(sess, dtype, op):
    """rows whose result is exactly the type's minimum and exactly its maximum, in an array that overflows nowhere: both routes
    give the model's bytes.  Then one slot at a time becomes the first value past the maximum and the first below the minimum — the
    first row, the last row of the ragged tail, lane 63 of a chunk, and a slot under a null — and both routes give the model's
    status: an error for a valid slot where the reference's test sees it (add: past the maximum, subtract: below the minimum,
    multiply: either), none under a null for add and subtract, an error under a null for multiply"""
    dt = np.dtype(dtype)
    lo, hi = M.limits(dt)
    n = ROWS[-1]
    rng = np.random.default_rng(90 + dt.itemsize)
    a, b = in_range_pairs(rng, dt, op, n)
    up, down, past_max, below_min = boundary_pairs(dt, op)
    spots = [0, 5, 62, 64, 700, 1023, 1024, n - 2]     # rows 0, 63, n − 1 and the null slot stay free for the flips
    for j, row in enumerate(spots):
        pairs = up if j % 2 == 0 else down
        a[row], b[row] = pairs[(j // 2) % len(pairs)]
    null_row = 900
    valid = rng.random(n) >= 0.2
    valid[[0, 63, n - 1] + spots] = True
    valid[null_row] = False
    text = f"{op}($0,$1)"

    def run(a, b, what):
        return check(sess, text, [Col(a, valid, 7, seed=1), Col(b, None, 65, seed=2)], (), (dtype, what))

    mv, mk, status = run(a, b, "in range")
    assert status == "ok"
    assert (mv[mk] == hi).any() and (mv[mk] == lo).any(), "the in-range array must hold exact-max and exact-min results"
    want_error = {"add": (True, False), "subtract": (False, True), "multiply": (True, True)}[op]
    for pair, direction, reports in ((past_max, "past max", want_error[0]), (below_min, "below min", want_error[1])):
        if pair is None:      # an unsigned type cannot get there
            continue
        for row in (0, n - 1, 63, null_row):
            a2, b2 = a.copy(), b.copy()
            a2[row], b2[row] = pair
            mv2, _, status = run(a2, b2, (direction, row))
            under_null = row == null_row
            expect = "overflow" if (reports and (op == "multiply" or not under_null)) else "ok"
            assert status == expect, (dtype, op, direction, row, "the model's own status")
            if status == "ok" and under_null:
                assert mv2[row] == 0
    # the same through a literal: the flip as a kernel argument
    (x, k_ok), (_, k_bad) = (down[0], below_min) if op == "subtract" else (up[0], past_max)
    col = np.full(n, x, dt)
    for lit, expect in ((k_ok, "ok"), (k_bad, "overflow")):
        _, _, status = check(sess, f"{op}($0,#0)", [Col(col, valid, 63, seed=3)], [(dtype, lit)], (dtype, "literal", lit))
        assert status == expect


# ---- lanes that hold no row -----------------------------------------------------------------------------------
EMPTY_LANE_TREES = ["multiply(add_unchecked($0,#0),#1)", "multiply(#1,subtract_unchecked($0,#0))", "multiply(add_unchecked($0,#0),add_unchecked($1,#1))"]


@pytest.mark.parametrize("dtype", ["int8", "int32", "int64", "uint16"])
def test_checked_multiply_ignores_lanes_without_a_row(sess, dtype):
    """the lanes past the last row, and all 64 lanes of an inactive unrolled step, hold 0 for every column and the literals' own
    values: a checked multiply whose literals alone would overflow must not report from there.  Every real row is in range, so
    both routes succeed with the model's values.  n = 1: a ragged chunk; n = 64: a full chunk, inactive steps only; n = 65: both"""
    dt = np.dtype(dtype)
    lo, hi = M.limits(dt)
    big = hi // 2 + 1                      # big · 2 and big · big are outside the type
    wrap = lambda v: v % (hi + 1) if lo == 0 else v   # noqa: E731
    for n in (1, 64, 65):
        valid = np.random.default_rng(n).random(n) >= 0.2
        # ($0 + big) · 2 with $0 + big = 1 in every row (wrapping, for the unsigned type); a lane without a row has big · 2
        c = Col(np.full(n, wrap(1 - big), dt), valid, 7, seed=1)
        mv, _, status = check(sess, EMPTY_LANE_TREES[0], [c], [(dtype, big), (dtype, 2)], (dtype, n))
        assert status == "ok" and (mv == 2).all()
        # 2 · ($0 − #0) with $0 − #0 = 3 in every row; a lane without a row has 2 · (0 − #0) = 2 · big (Uint16: 0 − big wraps to big)
        lit = big if lo == 0 else -big
        c = Col(np.full(n, lit + 3, dt), valid, 63, seed=2)
        mv, _, status = check(sess, EMPTY_LANE_TREES[1], [c], [(dtype, lit), (dtype, 2)], (dtype, n))
        assert status == "ok" and (mv == 6).all()
        # ($0 + big) · ($1 + big) = 3 · 2 in every row; a lane without a row has big · big
        ca, cb = Col(np.full(n, wrap(3 - big), dt), valid, 1, seed=3), Col(np.full(n, wrap(2 - big), dt), None, 65, seed=4)
        mv, _, status = check(sess, EMPTY_LANE_TREES[2], [ca, cb], [(dtype, big), (dtype, big)], (dtype, n))
        assert status == "ok" and (mv == 6).all()


# ---- null literals --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["int8", "uint16", "int64", "float32"])
def test_null_literals(sess, dtype):
    """a null literal makes every slot null.  The routes must agree on everything (check() compares them); the model decides the
    type, the validity and the status, and the values where its rules do: add holds 0 under a null, multiply computes every slot
    with the null scalar's payload (0).  What a comparison leaves in the data bits under an all-null validity is the routes' own"""
    for turn, n in enumerate(ROWS):
        cols = columns(dtype, n, turn, k=1)
        for text, by_model in (("greater($0,#0)", False), ("add($0,#0)", True), ("multiply($0,#0)", True), ("multiply(#0,$0)", True)):
            by_model = by_model and np.dtype(dtype).kind != "f"   # a float add has no slot rule: it is the unchecked kernel
            mv, mk, status = check(sess, text, cols, [(dtype, None)], (dtype, n), model_values=by_model)
            assert status == "ok" and not mk.any()
            if by_model:
                assert (mv == 0).all()
