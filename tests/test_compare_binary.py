"""equal / not_equal / less / less_equal / greater / greater_equal for String, Binary, LargeString, LargeBinary, FixedSizeBinary,
Decimal128 and Decimal256 operands (the base-binary, FixedSizeBinary and decimal kernels of CompareKernels,
arrow/compute/internal/kernels/scalar_comparisons.go:694-713, and compareFunction.DispatchBest, compute/scalar_compare.go:37-63).

The reference's CompareStringSuite, CompareFixedSizeBinary and CompareDecimalSuite tables are copied verbatim; everything else is
checked against a short restatement of bytes.Compare / signed decimal comparison below — the WHOLE data bitmap (bits under null
slots included) and the validity — and, outside quirk 10, against pyarrow.compute."""
import ctypes
import decimal
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

FUNCS = ("equal", "not_equal", "less", "less_equal", "greater", "greater_equal")
BASE_BINARY = (pa.string(), pa.binary(), pa.large_string(), pa.large_binary())
IDS = {"utf8": 13, "binary": 14, "fsb": 15, "d128": 23, "d256": 24, "large_utf8": 34, "large_binary": 35, "double": 12, "int64": 9,
       "bool": 1}


# ---- no GPU needed ------------------------------------------------------------------------------------------------
def test_compare_entry_points_are_declared_and_exported():
    from arrow_go_amd import _native as N
    from arrow_go_amd import compute as ac
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for sym in ("ah_compare_binary", "ah_compare_decimal"):
        assert sym in N.declared_symbols() and sym in exported, sym
    lib_c = ac.lib._name
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_c], text=True)
    assert "ahc_scalar_bytes" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    with open(N.HEADER_PATH.replace("arrowhip.h", "arrowhip_compute.h")) as f:
        assert "int ahc_scalar_bytes(" in f.read()


def _dispatch(fn, a, b):
    from arrow_go_amd import compute as ac
    tin, tout, err = (ctypes.c_int * 2)(a, b), (ctypes.c_int * 2)(), ctypes.create_string_buffer(512)
    rc = ac.lib.ahc_dispatch_best(fn.encode(), 2, tin, tout, err, len(err))
    return rc, (tout[0], tout[1]), err.value.decode()


# the binary and decimal rows of TestCompareKernelsDispatchBest (compute/scalar_compare_test.go:1258-1319), by type id
DISPATCH_ROWS = [
    ("utf8", "binary", "binary", "binary"),
    ("large_utf8", "binary", "large_binary", "large_binary"),
    ("large_utf8", "fsb", "large_binary", "large_binary"),
    ("binary", "fsb", "binary", "binary"),
    ("fsb", "fsb", "fsb", "fsb"),
    ("d128", "d128", "d128", "d128"),
    ("d128", "d256", "d256", "d256"),
    ("d128", "double", "double", "double"),
    ("double", "d128", "double", "double"),
    ("d128", "int64", "d128", "d128"),
    ("int64", "d128", "d128", "d128"),
]


@pytest.mark.parametrize("fn", FUNCS)
def test_dispatch_best_binary_and_decimal_rows(fn):
    for l, r, el, er in DISPATCH_ROWS:
        rc, got, err = _dispatch(fn, IDS[l], IDS[r])
        assert rc == 0, (fn, l, r, err)
        assert got == (IDS[el], IDS[er]), (fn, l, r, got)


@pytest.mark.parametrize("fn", FUNCS)
def test_dispatch_best_refuses_bool_with_string(fn):
    rc, _, err = _dispatch(fn, IDS["bool"], IDS["utf8"])
    assert rc != 0 and "has no kernel matching input types" in err


# ---- the restatement --------------------------------------------------------------------------------------------------
def _order(a, b):
    """bytes.Compare (unsigned, bytewise, a proper prefix first) or a signed value comparison: −1 / 0 / 1"""
    return (a > b) - (a < b)


def _decide(fn, c):
    return {"equal": c == 0, "not_equal": c != 0, "less": c < 0, "less_equal": c <= 0, "greater": c > 0, "greater_equal": c >= 0}[fn]


def raw_slots(x):
    """every slot's comparable value, validity ignored: bytes of base-binary / FixedSizeBinary slots (what the buffers hold, null
    slots included), the unscaled integer of a decimal slot.  A scalar: its value, a null scalar b"" / 0."""
    if isinstance(x, pa.Scalar):
        if pa.types.is_decimal(x.type):
            if not x.is_valid:
                return 0
            d = x.as_py()
            return int(d.scaleb(x.type.scale, context=decimal.Context(prec=100)))
        if not x.is_valid:
            return b""
        v = x.as_py()
        return v.encode() if isinstance(v, str) else bytes(v)
    t = x.type
    bufs = x.buffers()
    if pa.types.is_fixed_size_binary(t) or pa.types.is_decimal(t):
        w = t.byte_width
        data = bufs[1].to_pybytes() if bufs[1] is not None else b""
        out = []
        for i in range(x.offset, x.offset + len(x)):
            b = data[i * w:(i + 1) * w]
            out.append(int.from_bytes(b, "little", signed=True) if pa.types.is_decimal(t) else b)
        return out
    ow = 8 if t in (pa.large_string(), pa.large_binary()) else 4
    offs = np.frombuffer(bufs[1], dtype=np.int64 if ow == 8 else np.int32)
    data = bufs[2].to_pybytes() if bufs[2] is not None else b""
    return [data[offs[i]:offs[i + 1]] for i in range(x.offset, x.offset + len(x))]


def _scale(x):
    return x.type.scale if pa.types.is_decimal(x.type) else 0


def restate(fn, a, b, n):
    """(data bits over every slot, validity) of fn(a, b) — NullIntersection, a null scalar compared as empty bytes / zero"""
    ra, rb = raw_slots(a), raw_slots(b)
    if pa.types.is_decimal(a.type) or pa.types.is_decimal(b.type):
        s = max(_scale(a), _scale(b))
        fa, fb = 10 ** (s - _scale(a)), 10 ** (s - _scale(b))
        ra = [v * fa for v in ra] if isinstance(ra, list) else ra * fa
        rb = [v * fb for v in rb] if isinstance(rb, list) else rb * fb
    data, valid = [], []
    for i in range(n):
        x = ra[i] if isinstance(ra, list) else ra
        y = rb[i] if isinstance(rb, list) else rb
        data.append(_decide(fn, _order(x, y)))
        va = a.is_valid if isinstance(a, pa.Scalar) else a[i].is_valid
        vb = b.is_valid if isinstance(b, pa.Scalar) else b[i].is_valid
        valid.append(va and vb)
    return data, valid


def _bits(buf, off, n):
    if buf is None:
        return None
    raw = np.frombuffer(buf, dtype=np.uint8)
    return [bool((raw[(off + i) >> 3] >> ((off + i) & 7)) & 1) for i in range(n)]


def whole(res):
    """(data bits, validity) of a boolean result array, bits under null slots included"""
    n = len(res)
    bufs = res.buffers()
    v = _bits(bufs[0], res.offset, n)
    return _bits(bufs[1], res.offset, n), v if v is not None else [True] * n


def check(sess, fn, a, b, against_pyarrow=True):
    got = sess.call_function(fn, [a, b])
    n = len(a) if not isinstance(a, pa.Scalar) else len(b)
    assert len(got) == n
    exp_d, exp_v = restate(fn, a, b, n)
    gd, gv = whole(got)
    assert gv == exp_v, (fn, a.type, b.type)
    assert gd == exp_d, (fn, a.type, b.type)
    if against_pyarrow:
        assert got.to_pylist() == getattr(pc, fn)(a, b).to_pylist(), (fn, a.type, b.type)
    return got


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.close()


def _b(v):
    return [None if x is None else (x.encode() if isinstance(x, str) else x) for x in v]


def _arr(typ, vals):
    if typ in (pa.binary(), pa.large_binary()) or pa.types.is_fixed_size_binary(typ):
        return pa.array(_b(vals), type=typ)
    return pa.array(vals, type=typ)


def _sc(typ, v):
    if v is not None and (typ in (pa.binary(), pa.large_binary()) or pa.types.is_fixed_size_binary(typ)):
        v = v.encode()
    return pa.scalar(v, type=typ)


def _bools(txt):
    return [None if t.strip() == "null" else t.strip() == "true" for t in txt.strip("[]").split(",") if t.strip()]


# CompareStringSuite.TestSimpleCompareArrayScalar (scalar_compare_test.go:1169-1200)
STRING_AS = [
    ("equal", [], []),
    ("equal", [None], [None]),
    ("equal", ["zero", "zero", "one", "one", "two", "two"], [False, False, True, True, False, False]),
    ("equal", ["zero", "one", "two", "three", "four", "five"], [False, True, False, False, False, False]),
    ("equal", ["five", "four", "three", "two", "one", "zero"], [False, False, False, False, True, False]),
    ("equal", [None, "zero", "one", "one"], [None, False, True, True]),
    ("not_equal", [], []),
    ("not_equal", [None], [None]),
    ("not_equal", ["zero", "zero", "one", "one", "two", "two"], [True, True, False, False, True, True]),
    ("not_equal", ["zero", "one", "two", "three", "four", "five"], [True, False, True, True, True, True]),
    ("not_equal", ["five", "four", "three", "two", "one", "zero"], [True, True, True, True, False, True]),
    ("not_equal", [None, "zero", "one", "one"], [None, True, False, False]),
]


@pytest.mark.gpu
def test_reference_string_suite(sess):
    one = pa.scalar("one")
    for fn, vals, exp in STRING_AS:
        assert sess.call_function(fn, [pa.array(vals, pa.string()), one]).to_pylist() == exp, (fn, vals)
    na = pa.scalar(None, pa.string())
    col = pa.array([None, "zero", "one", "one"], pa.string())
    assert sess.call_function("equal", [col, na]).to_pylist() == [None] * 4
    assert sess.call_function("equal", [na, col]).to_pylist() == [None] * 4
    # TestRandomCompareArrayArray: random strings of 0..16 bytes, lengths 64 and 256, every null probability, EQ / NE
    rng = np.random.default_rng(0x5416447)
    for i in (3, 4):
        n = (1 << i) << i
        for p in (0.0, 0.01, 0.1, 0.25, 0.5, 1.0):
            cols = []
            for _ in range(2):
                vals = ["".join(chr(97 + c) for c in rng.integers(0, 3, rng.integers(0, 17))) for _ in range(n)]
                cols.append(pa.array([None if rng.random() < p else v for v in vals], pa.string()))
            for fn in ("equal", "not_equal"):
                check(sess, fn, cols[0], cols[1])


# CompareFixedSizeBinary (scalar_compare_test.go:841-1163): result tables and type pairings
T3, T1 = pa.binary(3), pa.binary(1)
FSB_AS = {"equal": ["[false, true, false, null]", "[false, false, false, null]", "[false, false, false, null]"],
          "not_equal": ["[true, false, true, null]", "[true, true, true, null]", "[true, true, true, null]"],
          "less": ["[true, false, false, null]", "[true, true, true, null]", "[true, false, false, null]"],
          "less_equal": ["[true, true, false, null]", "[true, true, true, null]", "[true, false, false, null]"],
          "greater": ["[false, false, true, null]", "[false, false, false, null]", "[false, true, true, null]"],
          "greater_equal": ["[false, true, true, null]", "[false, false, false, null]", "[false, true, true, null]"]}
FSB_SA = {"equal": ["[false, true, false, null]", "[false, false, false, null]", "[false, false, false, null]"],
          "not_equal": ["[true, false, true, null]", "[true, true, true, null]", "[true, true, true, null]"],
          "less": ["[false, false, true, null]", "[false, true, true, null]", "[false, false, false, null]"],
          "less_equal": ["[false, true, true, null]", "[false, true, true, null]", "[false, false, false, null]"],
          "greater": ["[true, false, false, null]", "[true, false, false, null]", "[true, true, true, null]"],
          "greater_equal": ["[true, true, false, null]", "[true, false, false, null]", "[true, true, true, null]"]}
FSB_AA = {"equal": ["[true, false, false, null, null]"] * 4 + ["[false, false, false, null, null]"] * 2,
          "not_equal": ["[false, true, true, null, null]"] * 4 + ["[true, true, true, null, null]"] * 2,
          "less": ["[false, true, false, null, null]", "[false, false, true, null, null]", "[false, true, false, null, null]",
                   "[false, false, true, null, null]", "[false, true, true, null, null]", "[true, true, false, null, null]"],
          "less_equal": ["[true, true, false, null, null]", "[true, false, true, null, null]", "[true, true, false, null, null]",
                         "[true, false, true, null, null]", "[false, true, true, null, null]", "[true, true, false, null, null]"],
          "greater": ["[false, false, true, null, null]", "[false, true, false, null, null]", "[false, false, true, null, null]",
                      "[false, true, false, null, null]", "[true, false, false, null, null]", "[false, false, true, null, null]"],
          "greater_equal": ["[true, false, true, null, null]", "[true, true, false, null, null]", "[true, false, true, null, null]",
                            "[true, true, false, null, null]", "[true, false, false, null, null]", "[false, false, true, null, null]"]}
OTHERS = (pa.binary(), pa.large_binary(), pa.string(), pa.large_string())
L1, R1 = ["aba", "abc", "abd", None], "abc"
L2, R2 = ["a", "b", "c", None], "b"
FSB_AS_TYPES = [(T3, T3, L1, R1, 0), (T1, T1, L2, R2, 0), (T3, T1, L1, R2, 1), (T1, T3, L2, R1, 2)] + \
               [p for o in OTHERS for p in ((T3, o, L1, R1, 0), (o, T3, L1, R1, 0))]
FSB_SA_TYPES = [(T3, T3, R1, L1, 0), (T1, T1, R2, L2, 0), (T3, T1, R1, L2, 1), (T1, T3, R2, L1, 2)] + \
               [p for o in OTHERS for p in ((T3, o, R1, L1, 0), (o, T3, R1, L1, 0))]
A1 = ["abc", "abc", "abd", None, "abc"]
B1 = ["abc", "abd", "abc", "abc", None]
A2 = ["a", "a", "d", None, "a"]
B2 = ["a", "d", "c", "a", None]
FSB_AA_TYPES = [(T3, T3, A1, B1, 0), (T3, T3, B1, A1, 1), (T1, T1, A2, B2, 2), (T1, T1, B2, A2, 3), (T3, T1, A1, B2, 4),
                (T1, T3, A2, B1, 5)] + [p for o in OTHERS for p in ((T3, o, A1, B1, 0), (o, T3, A1, B1, 0))]


@pytest.mark.gpu
@pytest.mark.parametrize("fn", FUNCS)
def test_reference_fixed_size_binary_suite(sess, fn):
    for lt, rt, lv, rv, k in FSB_AS_TYPES:
        assert sess.call_function(fn, [_arr(lt, [None]), pa.scalar(None, rt)]).to_pylist() == [None]
        assert sess.call_function(fn, [_arr(lt, lv), _sc(rt, rv)]).to_pylist() == _bools(FSB_AS[fn][k]), ("as", lt, rt)
        check(sess, fn, _arr(lt, lv), _sc(rt, rv), against_pyarrow=False)
    for lt, rt, lv, rv, k in FSB_SA_TYPES:
        assert sess.call_function(fn, [pa.scalar(None, lt), _arr(rt, [None])]).to_pylist() == [None]
        assert sess.call_function(fn, [_sc(lt, lv), _arr(rt, rv)]).to_pylist() == _bools(FSB_SA[fn][k]), ("sa", lt, rt)
        check(sess, fn, _sc(lt, lv), _arr(rt, rv), against_pyarrow=False)
    for lt, rt, lv, rv, k in FSB_AA_TYPES:
        assert sess.call_function(fn, [_arr(lt, []), _arr(rt, [])]).to_pylist() == []
        assert sess.call_function(fn, [_arr(lt, [None]), _arr(rt, [None])]).to_pylist() == [None]
        assert sess.call_function(fn, [_arr(lt, lv), _arr(rt, rv)]).to_pylist() == _bools(FSB_AA[fn][k]), ("aa", lt, rt)
        check(sess, fn, _arr(lt, lv), _arr(rt, rv), against_pyarrow=False)


# CompareDecimalSuite (scalar_compare_test.go:636-839)
DEC_AS = {"equal": "[true, false, false, null]", "not_equal": "[false, true, true, null]", "less": "[false, false, true, null]",
          "less_equal": "[true, false, true, null]", "greater": "[false, true, false, null]", "greater_equal": "[true, true, false, null]"}
DEC_SA = {"equal": "[true, false, false, null]", "not_equal": "[false, true, true, null]", "less": "[false, true, false, null]",
          "less_equal": "[true, true, false, null]", "greater": "[false, false, true, null]", "greater_equal": "[true, false, true, null]"}
DEC_AA = {"equal": "[true, false, false, true, false, false, null, null]", "not_equal": "[false, true, true, false, true, true, null, null]",
          "less": "[false, true, false, false, true, false, null, null]", "less_equal": "[true, true, false, true, true, false, null, null]",
          "greater": "[false, false, true, false, false, true, null, null]",
          "greater_equal": "[true, false, true, true, false, true, null, null]"}
DEC_DIFF = {"equal": "[true, false, false, true, false, false]", "not_equal": "[false, true, true, false, true, true]",
            "less": "[false, true, false, false, true, false]", "less_equal": "[true, true, false, true, true, false]",
            "greater": "[false, false, true, false, false, true]", "greater_equal": "[true, false, true, true, false, true]"}
D = decimal.Decimal


def _dec(t, vals):
    return pa.array([None if v is None else D(v) for v in vals], type=t)


def _refused(sess, fn, a, b):
    from arrow_go_amd import compute as ac
    with pytest.raises(ac.ErrNotImplemented, match="unsupported cast to"):
        sess.call_function(fn, [a, b])


@pytest.mark.gpu
@pytest.mark.parametrize("width", [128, 256])
@pytest.mark.parametrize("fn", FUNCS)
def test_reference_decimal_suite(sess, fn, width):
    ty = pa.decimal128(3, 2) if width == 128 else pa.decimal256(3, 2)
    # TestArrayScalar
    lhs = _dec(ty, ["1.23", "2.34", "-1.23", None])
    lhs_f = pa.array([1.23, 2.34, -1.23, None], pa.float64())
    lhs_int_like = _dec(ty, ["1.00", "2.00", "-1.00", None])
    rhs = pa.scalar(D("1.23"), ty)
    assert sess.call_function(fn, [lhs, rhs]).to_pylist() == _bools(DEC_AS[fn])
    _refused(sess, fn, lhs_f, rhs)
    _refused(sess, fn, lhs, pa.scalar(1.23))
    assert sess.call_function(fn, [lhs_int_like, pa.scalar(1, pa.int64())]).to_pylist() == _bools(DEC_AS[fn])
    # TestScalarArray
    assert sess.call_function(fn, [rhs, lhs]).to_pylist() == _bools(DEC_SA[fn])
    _refused(sess, fn, rhs, lhs_f)
    _refused(sess, fn, pa.scalar(1.23), lhs)
    assert sess.call_function(fn, [pa.scalar(1, pa.int64()), lhs_int_like]).to_pylist() == _bools(DEC_SA[fn])
    # TestArrayArray
    l8 = _dec(ty, ["1.23", "1.23", "2.34", "-1.23", "-1.23", "1.23", "1.23", None])
    r8 = _dec(ty, ["1.23", "2.34", "1.23", "-1.23", "1.23", "-1.23", None, "1.23"])
    assert sess.call_function(fn, [_dec(ty, []), _dec(ty, [])]).to_pylist() == []
    assert sess.call_function(fn, [_dec(ty, [None]), _dec(ty, [None])]).to_pylist() == [None]
    assert sess.call_function(fn, [l8, r8]).to_pylist() == _bools(DEC_AA[fn])
    _refused(sess, fn, pa.array([1.23, 1.23, 2.34, -1.23, -1.23, 1.23, 1.23, None]), r8)
    _refused(sess, fn, l8, pa.array([1.23, 2.34, 1.23, -1.23, 1.23, -1.23, None, 1.23]))
    _refused(sess, fn, _dec(ty, ["1.00", "1.00", "2.00", "-1.00", "-1.00", "1.00", "1.00", None]),
             pa.array([1, 2, 1, -1, 1, -1, None, 1], pa.int64()))
    # TestDiffParams
    ty2 = pa.decimal128(4, 3) if width == 128 else pa.decimal256(4, 3)
    l6 = _dec(ty, ["1.23", "1.23", "2.34", "-1.23", "-1.23", "1.23"])
    r6 = _dec(ty2, ["1.230", "2.340", "1.230", "-1.230", "1.230", "-1.230"])
    assert sess.call_function(fn, [l6, r6]).to_pylist() == _bools(DEC_DIFF[fn])
    check(sess, fn, l6, r6)


# ---- against the restatement ---------------------------------------------------------------------------------------
def _rand_values(rng, n, lo=0, hi=12, alphabet=(0x00, 0x61, 0x62, 0x80, 0xFF), null_p=0.2):
    out = []
    for _ in range(n):
        if rng.random() < null_p:
            out.append(None)
        else:
            out.append(bytes(rng.choice(alphabet, rng.integers(lo, hi + 1)).astype(np.uint8).tobytes()))
    return out


def _typed(typ, vals):
    """bytes values as a column of `typ` (strings: only when the bytes are UTF-8 — the alphabets below keep them so)"""
    if typ in (pa.string(), pa.large_string()):
        return pa.array([None if v is None else v.decode("latin-1") for v in vals], type=typ)
    return pa.array(vals, type=typ)


UTF8_SAFE = (0x00, 0x61, 0x62, 0x7F)


@pytest.mark.gpu
@pytest.mark.parametrize("lt", BASE_BINARY)
@pytest.mark.parametrize("rt", BASE_BINARY)
def test_base_binary_pairings_all_shapes(sess, lt, rt):
    rng = np.random.default_rng(BASE_BINARY.index(lt) * 4 + BASE_BINARY.index(rt))
    safe = lt in (pa.string(), pa.large_string()) or rt in (pa.string(), pa.large_string())
    alpha = UTF8_SAFE if safe else (0x00, 0x61, 0x62, 0x80, 0xFF)
    n = 300
    a = _typed(lt, _rand_values(rng, n, alphabet=alpha))
    b = _typed(rt, _rand_values(rng, n, alphabet=alpha))
    sa = _typed(lt, _rand_values(rng, 1, null_p=0, alphabet=alpha))[0]
    sb = _typed(rt, _rand_values(rng, 1, null_p=0, alphabet=alpha))[0]
    for fn in FUNCS:
        same = lt == rt
        check(sess, fn, a, b, against_pyarrow=same)
        check(sess, fn, a, sb, against_pyarrow=same)
        check(sess, fn, sa, b, against_pyarrow=same)
        check(sess, fn, a, pa.scalar(None, rt), against_pyarrow=False)
        check(sess, fn, pa.scalar(None, lt), b, against_pyarrow=False)


@pytest.mark.gpu
def test_mixed_pairings_with_fixed_size_binary(sess):
    rng = np.random.default_rng(7)
    n = 200
    for w in (1, 3, 8, 16, 20):
        f = pa.array([None if rng.random() < 0.2 else bytes(rng.choice(UTF8_SAFE, w).astype(np.uint8)) for _ in range(n)], pa.binary(w))
        for other in (pa.binary(2), pa.binary(16)) + BASE_BINARY:
            if pa.types.is_fixed_size_binary(other):
                ow = other.byte_width
                o = pa.array([None if rng.random() < 0.2 else bytes(rng.choice(UTF8_SAFE, ow).astype(np.uint8)) for _ in range(n)], other)
            else:
                o = _typed(other, _rand_values(rng, n, lo=0, hi=20, alphabet=UTF8_SAFE))
            for fn in FUNCS:
                check(sess, fn, f, o, against_pyarrow=False)
                check(sess, fn, o, f, against_pyarrow=False)
                check(sess, fn, f, o[3] if o[3].is_valid else o[4], against_pyarrow=False)
                check(sess, fn, o[5] if o[5].is_valid else o[6], f, against_pyarrow=False)


@pytest.mark.gpu
def test_less_is_flipped_greater(sess):
    rng = np.random.default_rng(11)
    a = pa.array(_rand_values(rng, 500), pa.binary())
    b = pa.array(_rand_values(rng, 500), pa.binary())
    for lo, hi in (("less", "greater"), ("less_equal", "greater_equal")):
        x, y = sess.call_function(lo, [a, b]), sess.call_function(hi, [b, a])
        assert whole(x) == whole(y)


@pytest.mark.gpu
def test_empty_against_null_and_high_bytes(sess):
    a = pa.array([b"", b"", None, b"\x80", b"\xff", b"\x7f", b"ab", b"ab\x00", b"abc"], pa.binary())
    b = pa.array([None, b"", b"", b"\x7f", b"\xff\x00", b"\x80", b"ab\x00", b"ab", b"ab\x00"], pa.binary())
    for fn in FUNCS:
        check(sess, fn, a, b)
        check(sess, fn, a, pa.scalar(b"", pa.binary()))
        check(sess, fn, a, pa.scalar(None, pa.binary()), against_pyarrow=False)


@pytest.mark.gpu
@pytest.mark.parametrize("typ", [pa.binary(), pa.large_string()])
def test_long_values_and_shared_prefixes(sess, typ):
    """65-byte and 4 KiB values, 64-byte shared prefixes that differ just after, and neighbours of every length"""
    rng = np.random.default_rng(3)
    prefix = b"a" * 64
    vals_a, vals_b = [], []
    for i in range(700):
        k = i % 7
        if k == 0:
            x = prefix + bytes([0x61 + rng.integers(0, 2)])  # 65 bytes
            y = prefix + bytes([0x61 + rng.integers(0, 2)])
        elif k == 1:
            x = bytes(rng.choice(UTF8_SAFE, 4096).astype(np.uint8))
            y = bytearray(x)
            if rng.random() < 0.5:
                y[rng.integers(0, 4096)] = 0x62
            y = bytes(y)
        elif k == 2:
            x = prefix * 8 + b"z" * int(rng.integers(0, 3))
            y = prefix * 8 + b"z" * int(rng.integers(0, 3))
        elif k == 3:
            x, y = prefix * 3, prefix * 3 + b"\x00"
        else:
            x, y = bytes(rng.choice(UTF8_SAFE, rng.integers(0, 10)).astype(np.uint8)), b"ab"
        vals_a.append(None if rng.random() < 0.05 else x)
        vals_b.append(y)
    a, b = _typed(typ, vals_a), _typed(typ, vals_b)
    long_scalar = _typed(typ, [vals_b[1]])[0]
    for fn in FUNCS:
        check(sess, fn, a, b)
        check(sess, fn, a, long_scalar)
        check(sess, fn, _typed(typ, [prefix * 70]), _typed(typ, [prefix * 70 + b"a"])[0])  # a 4480-byte scalar: read from HBM
        check(sess, fn, _typed(typ, [prefix * 70] * 3), _typed(typ, [prefix * 70 + b"a", prefix * 70, prefix * 69])[0])


@pytest.mark.gpu
def test_lengths_around_64_row_boundaries_and_slices(sess):
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 127, 128, 129, 1000):
        a = pa.array(_rand_values(rng, n + 9, hi=4), pa.large_binary())
        b = pa.array(_rand_values(rng, n + 9, hi=4), pa.binary())
        for off in (0, 1, 7, 9):
            x, y = a.slice(off, n), b.slice(9 - off, n)
            for fn in FUNCS:
                check(sess, fn, x, y, against_pyarrow=False)
                check(sess, fn, x, pa.scalar(b"ab", pa.binary()), against_pyarrow=False)


@pytest.mark.gpu
def test_sliced_fixed_size_binary_honours_offset(sess):
    """quirk 10: the reference's FSBIter ignores the span offset; Arrow C++ and this layer honour it"""
    rng = np.random.default_rng(9)
    a = pa.array([bytes(rng.choice(UTF8_SAFE, 4).astype(np.uint8)) for _ in range(300)], pa.binary(4))
    b = pa.array([bytes(rng.choice(UTF8_SAFE, 4).astype(np.uint8)) for _ in range(300)], pa.binary(4))
    for off, n in ((1, 100), (13, 200), (64, 64), (65, 3)):
        for fn in FUNCS:
            check(sess, fn, a.slice(off, n), b.slice(300 - n - 5, n))  # pyarrow: second check
            check(sess, fn, a.slice(off, n), b[0])


@pytest.mark.gpu
def test_output_bit_offsets_through_the_raw_entry_point():
    """ah_compare_binary writes bits [k, k + n) and keeps every other bit, for k = 0 … 7 and k = 70"""
    import arrow_go_amd as ah
    vals_a = [b"", b"a", b"ab", b"b", b"\xff", b"abc" * 30, b"x"] * 20
    vals_b = [b"", b"b", b"ab", b"a", b"\x00", b"abc" * 30, b"xy"] * 20
    n = len(vals_a)

    def enc(vals):
        offs = np.zeros(len(vals) + 1, np.int32)
        offs[1:] = np.cumsum([len(v) for v in vals])
        return offs, np.frombuffer(b"".join(vals) + b"\0" * 8, np.uint8)

    with ah.Context(0) as ctx:
        oa, da = enc(vals_a)
        ob, db = enc(vals_b)
        bufs = [ctx.to_device(x) for x in (oa, da, ob, db)]
        for k in list(range(8)) + [70]:
            for op, fn in enumerate(("equal", "not_equal", "greater", "greater_equal")):
                nbytes = (k + n + 7) // 8 + 8
                out = ctx.to_device(np.full(nbytes, 0xA5, np.uint8))
                ctx.compare_binary(op, (4, 0, bufs[0], bufs[1], 0, 0), (4, 0, bufs[2], bufs[3], 0, 0), n, out, k)
                got = np.unpackbits(out.download(np.uint8, nbytes), bitorder="little")
                keep = np.unpackbits(np.full(nbytes, 0xA5, np.uint8), bitorder="little")
                exp = keep.copy()
                exp[k:k + n] = [_decide(fn, _order(x, y)) for x, y in zip(vals_a, vals_b)]
                assert (got == exp).all(), (k, fn)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [128, 256])
def test_decimal_extremes_negatives_and_scale_promotion(sess, width):
    rng = np.random.default_rng(width)
    pmax = 38 if width == 128 else 76
    mk = pa.decimal128 if width == 128 else pa.decimal256
    big = 10 ** pmax - 1
    ints = [big, -big, 0, 1, -1, big - 1, -(big - 1), 10 ** (pmax - 1), -(10 ** (pmax - 1))]
    ints += [int(rng.integers(-10**18, 10**18)) * int(rng.integers(1, 10**18)) % big * (1 if rng.random() < 0.5 else -1) for _ in range(500)]
    t = mk(pmax, 0)
    a = pa.array([D(v) for v in ints], t)
    b = pa.array([D(v) for v in ints[1:] + ints[:1]], t)
    for fn in FUNCS:
        check(sess, fn, a, b)
        check(sess, fn, a, pa.scalar(D(ints[3]), t))
        check(sess, fn, a, pa.scalar(None, t), against_pyarrow=False)
    # scale promotion: (p, s) against (p + 3, s + 3), rescaled on the device
    t1, t2 = mk(20, 2), mk(23, 5)
    x = pa.array([None if rng.random() < 0.1 else D(int(rng.integers(-10**17, 10**17))).scaleb(-2) for _ in range(400)], t1)
    y = pa.array([D(int(v)).scaleb(-5) if i % 3 else (x[i].as_py() or D(0)) for i, v in enumerate(rng.integers(-10**17, 10**17, 400))], t2)
    for fn in FUNCS:
        check(sess, fn, x, y)
        check(sess, fn, y, x)
        check(sess, fn, x, pa.scalar(D("-12.34567"), t2))
    if width == 128:  # Decimal128 ∘ Decimal256 → Decimal256
        z = pa.array([None if v is None else v for v in y.to_pylist()], pa.decimal256(40, 5))
        for fn in FUNCS:
            check(sess, fn, x, z)
            check(sess, fn, z, x)


@pytest.mark.gpu
def test_decimal_precision_overflow_is_refused(sess):
    from arrow_go_amd import compute as ac
    a = pa.array([D(1)], pa.decimal128(38, 0))
    b = pa.array([D(1)], pa.decimal128(38, 10))
    with pytest.raises(ac.ErrInvalid, match=r"Decimal precision out of range \[1, 38\]: 48"):
        sess.call_function("equal", [a, b])
    a = pa.array([D(1)], pa.decimal256(76, 0))
    b = pa.array([D(1)], pa.decimal256(76, 10))
    with pytest.raises(ac.ErrInvalid, match=r"\[1, 76\]: 86"):
        sess.call_function("less", [a, b])


@pytest.mark.gpu
def test_large_column(sess):
    n = 1 << 20
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 24, n)
    pool = rng.integers(0x61, 0x64, int(lens.sum()) + 8).astype(np.uint8).tobytes()
    offs = np.zeros(n + 1, np.int32)
    offs[1:] = np.cumsum(lens)
    a = pa.Array.from_buffers(pa.string(), n, [None, pa.py_buffer(offs.tobytes()), pa.py_buffer(pool)])
    b = pc.utf8_reverse(a)
    for fn in ("equal", "less", "greater_equal"):
        got = sess.call_function(fn, [a, b])
        assert got.equals(getattr(pc, fn)(a, b)), fn
        got = sess.call_function(fn, [a, pa.scalar("abc")])
        assert got.equals(getattr(pc, fn)(a, pa.scalar("abc"))), fn


@pytest.mark.gpu
def test_chunked_and_record_batch_columns(sess):
    rng = np.random.default_rng(2)
    chunks = [pa.array(_rand_values(rng, n, alphabet=UTF8_SAFE), pa.binary()).cast(pa.string()) for n in (10, 0, 70, 129)]
    col = pa.chunked_array(chunks, pa.string())
    for fn in FUNCS:
        got = sess.call_function(fn, [col, pa.scalar("ab")])
        assert got.to_pylist() == getattr(pc, fn)(col, pa.scalar("ab")).to_pylist()
    other = pa.chunked_array([c for c in pc.utf8_reverse(col).chunks], pa.string())
    got = sess.call_function("less", [col, other])
    assert got.to_pylist() == pc.less(col, other).to_pylist()
    batch = pa.RecordBatch.from_arrays([col.combine_chunks(), other.combine_chunks()], names=["a", "b"])
    tree = ("call", "and_kleene", [("call", "less", [("field", "a"), ("field", "b")]), ("call", "not_equal", [("field", "a"), ("lit", pa.scalar(""))])])
    res, fused = sess.eval_expression_tree(tree, list(batch.columns), names=batch.schema.names, fuse=True)
    assert not fused
    exp = pc.and_kleene(pc.less(batch["a"], batch["b"]), pc.not_equal(batch["a"], pa.scalar("")))
    assert res.to_pylist() == exp.to_pylist()


@pytest.mark.gpu
def test_string_literal_expression_tree_equals_per_call(sess):
    rng = np.random.default_rng(4)
    a = pa.array(_rand_values(rng, 1000, hi=3, alphabet=UTF8_SAFE), pa.binary()).cast(pa.string())
    tree = ("call", "greater_equal", [("field", 0), ("lit", pa.scalar("a"))])
    res, fused = sess.eval_expression_tree(tree, [a], fuse=True)
    assert not fused
    per_call = sess.call_function("greater_equal", [a, pa.scalar("a")])
    assert whole(res) == whole(per_call)
    assert res.to_pylist() == pc.greater_equal(a, pa.scalar("a")).to_pylist()


@pytest.mark.gpu
def test_all_scalar_call_returns_a_scalar(sess):
    got = sess.call_function("less", [pa.scalar("ab"), pa.scalar(b"abc", pa.large_binary())])
    assert isinstance(got, pa.Scalar) and got.as_py() is True
    got = sess.call_function("equal", [pa.scalar(D("1.50"), pa.decimal128(5, 2)), pa.scalar(D("1.5"), pa.decimal256(4, 1))])
    assert got.as_py() is True
