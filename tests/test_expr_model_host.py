"""tests/expr_model.py held against the CPU oracle, op by op, on full-range inputs of all ten numeric types — no GPU.

The oracle (oracle/orc_arith.c, orc_bits.c through tests/oracle_lib.py) restates the reference's kernels in C and is itself held
against the reference's own machine code (tests/test_oracle_vs_reference.py); the model is numpy and Python integers.  They share no
code, so the model may serve as the yardstick of tests/test_expressions_ranges.py only as far as these tests reach: every fusible
arithmetic, unary and comparison op, array/array and array/scalar in both orders, validity at bit offsets, a valid and a null
scalar.  Results are compared bit for bit; a NaN result may differ in payload and sign only (same_bits_or_both_nan).
"""
import numpy as np
import pytest

from tests import oracle_lib as OL
from tests import expr_model as M
from tests.test_gpu_parity import rand, same_bits_or_both_nan

ADD, SUB, MUL = 0, 1, 2
ABS, NEGATE, SIGN = 4, 5, 20
AA, AS, SA = 0, 1, 2
STATUS = {0: "ok", 3: "overflow"}

SIZES = [1, 7, 64, 65, 1031]


@pytest.fixture(scope="module")
def orc():
    return OL.load_oracle()


boundary = M.boundary


def full_range(rng, dtype, n, shift=0):
    """rand() of test_gpu_parity with the boundary set planted from the first row on and up to the last row, rotated by `shift`
    so that two operands meet in different pairs"""
    a = rand(rng, dtype, n)
    b = np.roll(boundary(dtype), shift)
    k = min(len(b), n)
    a[:k] = b[:k]
    if n >= 2 * len(b):
        a[n - len(b):] = b[::-1]
    return a


def valid_bits(rng, n, off, p=0.8):
    bits = rng.random(off + n) < p
    return OL.pack_bits(bits), bits[off:off + n]


@pytest.mark.parametrize("dtype", OL.ALL_DTYPES, ids=str)
def test_model_unchecked_arithmetic_equals_oracle(orc, dtype):
    rng = np.random.default_rng(101 + OL.TYPE_IDS[np.dtype(dtype)])
    for n in SIZES:
        l, r = full_range(rng, dtype, n), full_range(rng, dtype, n, shift=3)
        for name, op in (("add_unchecked", ADD), ("subtract_unchecked", SUB), ("multiply_unchecked", MUL)):
            exp = orc.arithmetic(op, AA, l, r)
            got, valid, status = M.evaluate(f"{name}($0,$1)", [(l, None), (r, None)])
            assert got.dtype == exp.dtype and status == "ok" and valid.all()
            assert same_bits_or_both_nan(got, exp), (dtype, name, n)
            for s in boundary(dtype):
                sc = np.array([s], dtype)
                exp = orc.arithmetic(op, AS, l, sc)
                got, _, _ = M.evaluate(f"{name}($0,#0)", [(l, None)], [(dtype, s)])
                assert same_bits_or_both_nan(got, exp), (dtype, name, n, "array/scalar", s)
                exp = orc.arithmetic(op, SA, sc, r)
                got, _, _ = M.evaluate(f"{name}(#0,$0)", [(r, None)], [(dtype, s)])
                assert same_bits_or_both_nan(got, exp), (dtype, name, n, "scalar/array", s)


@pytest.mark.parametrize("dtype", OL.ALL_DTYPES, ids=str)
def test_model_unary_equals_oracle(orc, dtype):
    rng = np.random.default_rng(202)
    for n in SIZES:
        a = full_range(rng, dtype, n)
        for name, op in (("abs_unchecked", ABS), ("negate_unchecked", NEGATE), ("sign", SIGN)):
            exp = orc.arithmetic_unary(op, a)
            got, valid, status = M.evaluate(f"{name}($0)", [(a, None)])
            assert got.dtype == exp.dtype and status == "ok" and valid.all()
            assert same_bits_or_both_nan(got, exp), (dtype, name, n)
            if name == "sign" and np.dtype(dtype).kind == "f" and n >= 16:   # sign(±0) = +0 and sign(NaN) = NaN, by their bits
                zeros = a == 0
                assert zeros.any() and not np.signbit(got[zeros]).any() and np.isnan(got[np.isnan(a)]).all()


@pytest.mark.parametrize("dtype", OL.ALL_DTYPES, ids=str)
def test_model_checked_equals_oracle(orc, dtype):
    """status and bytes.  The bytes are compared whenever the oracle reports no error: with an error the reference's output is
    not defined (the call fails).  Full-range operands nearly always overflow, so each op also gets operands drawn so that few
    slots do, and the statuses seen are asserted to include both."""
    rng = np.random.default_rng(303 + OL.TYPE_IDS[np.dtype(dtype)])
    dt = np.dtype(dtype)
    seen = set()
    for n in SIZES:
        for loff, roff in ((0, 0), (5, 9), (63, 1)):
            lbits, lk = valid_bits(rng, n, loff)
            rbits, rk = valid_bits(rng, n, roff)
            for mode in ("full", "half", "small"):
                if mode == "full" or dt.kind == "f":
                    l, r = full_range(rng, dtype, n), full_range(rng, dtype, n, shift=2)
                elif mode == "half":   # sums and differences mostly in range, products mostly not
                    info = np.iinfo(dt)
                    l = rng.integers(info.min // 2, info.max // 2, n, dtype=dt, endpoint=True)
                    r = rng.integers(info.min // 2, info.max // 2, n, dtype=dt, endpoint=True)
                    if dt.kind == "u":
                        l, r = np.maximum(l, r), np.minimum(l, r)   # l − r stays at or above 0
                else:
                    l, r = rng.integers(6, 11, n).astype(dt), rng.integers(0, 6, n).astype(dt)
                for name, op in (("add", 21), ("subtract", 22), ("multiply", 23)):
                    st, exp = orc.arithmetic_checked(op, AA, l, lbits, loff, r, rbits, roff)
                    got, valid, status = M.evaluate(f"{name}($0,$1)", [(l, lk), (r, rk)])
                    assert status == STATUS[st], (dtype, name, n, loff, roff, mode)
                    assert (valid == (lk & rk)).all() and got.dtype == exp.dtype
                    seen.add((name, status))
                    if st == 0:
                        assert same_bits_or_both_nan(got, exp), (dtype, name, n, loff, roff, mode)
                    for s, sv in [(x, True) for x in boundary(dtype)[:7]] + [(0, False)]:
                        sc = np.array([s], dtype)
                        lit = (dtype, s if sv else None)
                        st, exp = orc.arithmetic_checked(op, AS, l, lbits, loff, sc, None, 0, scalar_valid=sv)
                        got, valid, status = M.evaluate(f"{name}($0,#0)", [(l, lk)], [lit])
                        assert status == STATUS[st] and (valid == (lk & sv)).all(), (dtype, name, n, mode, "array/scalar", s, sv)
                        if st == 0:
                            assert same_bits_or_both_nan(got, exp), (dtype, name, n, mode, "array/scalar", s, sv)
                        st, exp = orc.arithmetic_checked(op, SA, sc, None, 0, r, rbits, roff, scalar_valid=sv)
                        got, valid, status = M.evaluate(f"{name}(#0,$0)", [(r, rk)], [lit])
                        assert status == STATUS[st] and (valid == (rk & sv)).all(), (dtype, name, n, mode, "scalar/array", s, sv)
                        if st == 0:
                            assert same_bits_or_both_nan(got, exp), (dtype, name, n, mode, "scalar/array", s, sv)
    if dt.kind != "f":
        assert seen == {(name, st) for name in ("add", "subtract", "multiply") for st in ("ok", "overflow")}


@pytest.mark.parametrize("dtype", OL.INT_DTYPES, ids=str)
def test_model_checked_null_slots(orc, dtype):
    """the slot rule alone: the only out-of-range pair sits under a null → add and subtract stay silent and hold 0 there,
    multiply reports"""
    dt = np.dtype(dtype)
    info = np.iinfo(dt)
    n = 70
    for k in (0, 63, 69):
        valid = np.ones(n + 5, bool)
        valid[5 + k] = False
        bits = OL.pack_bits(valid)
        cases = {"add": (21, info.max, 1), "subtract": (22, info.min, 1), "multiply": (23, info.max, 2)}
        for name, (op, a, b) in cases.items():
            l, r = np.full(n, 7, dt), np.full(n, 3, dt)
            l[k], r[k] = a, b
            for lk in (valid[5:5 + n], None):
                st, exp = orc.arithmetic_checked(op, AA, l, bits if lk is not None else None, 5, r, None, 0)
                got, _, status = M.evaluate(f"{name}($0,$1)", [(l, lk), (r, None)])
                want = "overflow" if (lk is None or name == "multiply") else "ok"
                assert status == STATUS[st] == want, (dtype, name, k, lk is None)
                if st == 0:
                    assert got.tobytes() == exp.tobytes() and got[k] == 0


@pytest.mark.parametrize("dtype", OL.ALL_DTYPES, ids=str)
def test_model_comparisons_equal_oracle(orc, dtype):
    """the oracle has ==, !=, > and >= (the reference makes < and <= of them by exchanging the arguments); bits land at a bit offset"""
    rng = np.random.default_rng(404)
    base = {"equal": (0, False), "not_equal": (1, False), "greater": (2, False), "greater_equal": (3, False),
            "less": (2, True), "less_equal": (3, True)}
    for n in SIZES:
        l, r = full_range(rng, dtype, n), full_range(rng, dtype, n, shift=1)
        same = rng.random(n) < 0.3   # ties, beyond the planted ones
        r[same] = l[same]
        for name, (cmpop, flip) in base.items():
            for off in (0, 3):
                def want(shape, a, b):
                    if flip:
                        shape, a, b = {AA: AA, AS: SA, SA: AS}[shape], b, a
                    out = orc.comparison(cmpop, shape, a, b, np.zeros((off + n + 7) // 8 + 1, np.uint8), off)
                    return OL.unpack_bits(out, off, n)
                got, valid, status = M.evaluate(f"{name}($0,$1)", [(l, None), (r, None)])
                assert got.dtype == bool and status == "ok" and valid.all()
                assert (got == want(AA, l, r)).all(), (dtype, name, n)
                for s in boundary(dtype):
                    sc = np.array([s], dtype)
                    got, _, _ = M.evaluate(f"{name}($0,#0)", [(l, None)], [(dtype, s)])
                    assert (got == want(AS, l, sc)).all(), (dtype, name, n, "array/scalar", s)
                    got, _, _ = M.evaluate(f"{name}(#0,$0)", [(r, None)], [(dtype, s)])
                    assert (got == want(SA, sc, r)).all(), (dtype, name, n, "scalar/array", s)


def test_model_validity_and_boolean_ops():
    """what the oracle's arithmetic entry points do not carry: validity of unchecked ops and comparisons, null literals, and the
    four bitmap ops with invert — small enough to state by hand"""
    a = np.array([1, 2, 3, 4], np.int32)
    ak = np.array([True, False, True, True])
    b = np.array([4, 3, 2, 1], np.int32)
    bk = np.array([True, True, False, True])
    v, k, st = M.evaluate("greater(add_unchecked($0,$1),#0)", [(a, ak), (b, bk)], [(np.int32, 4)])
    assert v.tolist() == [True] * 4 and k.tolist() == [True, False, False, True] and st == "ok"
    v, k, st = M.evaluate("greater($0,#0)", [(a, None)], [(np.int32, None)])
    assert k.tolist() == [False] * 4 and st == "ok"
    v, k, st = M.evaluate("add($0,#0)", [(a, None)], [(np.int32, None)])
    assert v.tolist() == [0] * 4 and not k.any()
    x = np.array([True, True, False, False])
    y = np.array([True, False, True, False])
    for name, exp in (("and", [1, 0, 0, 0]), ("or", [1, 1, 1, 0]), ("xor", [0, 1, 1, 0]), ("and_not", [0, 1, 0, 0])):
        v, k, st = M.evaluate(f"{name}($0,$1)", [(x, ak), (y, bk)])
        assert v.tolist() == [bool(e) for e in exp] and k.tolist() == [True, False, False, True]
    v, k, _ = M.evaluate("invert(and_not($0,$1))", [(x, ak), (y, None)])
    assert v.tolist() == [True, False, True, True] and k.tolist() == ak.tolist()
    with pytest.raises(KeyError):
        M.evaluate("and_kleene($0,$1)", [(x, None), (y, None)])
    with pytest.raises(ValueError):
        M.parse("add($0,$1")


def test_model_promotion():
    """commonNumeric and the value-preserving rule, against the pairs test_fused_implicit_promotion runs and a few that must not fuse"""
    cn = M.common_numeric
    assert cn(np.int8, np.int64) == np.int64 and cn(np.uint16, np.int32) == np.int32 and cn(np.int8, np.uint16) == np.int32
    assert cn(np.uint32, np.uint64) == np.uint64 and cn(np.int32, np.uint32) == np.int64 and cn(np.int8, np.uint64) == np.int64
    assert cn(np.int32, np.float64) == np.float64 and cn(np.int16, np.float32) == np.float32 and cn(np.float32, np.float64) == np.float64
    vp = M.value_preserving
    assert vp(np.int8, np.int64) and vp(np.uint32, np.uint64) and vp(np.int32, np.float64) and vp(np.int16, np.float32) and vp(np.uint16, np.int32)
    assert not vp(np.int64, np.float64) and not vp(np.int32, np.float32) and not vp(np.int32, np.uint32) and not vp(np.uint64, np.int64)
    v, _, st = M.evaluate("add($0,$1)", [(np.array([-128], np.int8), None), (np.array([2**63 - 1], np.int64), None)])
    assert v.dtype == np.int64 and v.tolist() == [2**63 - 129] and st == "ok"
    v, _, _ = M.evaluate("less($0,#0)", [(np.array([-2**31], np.int32), None)], [(np.int64, 12345678901)])
    assert v.tolist() == [True]
    with pytest.raises(TypeError):
        M.evaluate("add($0,$1)", [(np.array([1], np.int64), None), (np.array([1.5]), None)])
    with pytest.raises(ValueError):
        M.evaluate("add($0,#0)", [(np.array([1.5]), None)], [(np.int64, 2**53 + 1)])
