"""is_in for String, Binary, LargeString, LargeBinary, FixedSizeBinary, Decimal128 / 256 and dictionary columns, with array
and chunked value sets (arrow/compute/scalar_set_lookup.go:175-232, kernels/scalar_set_lookup.go).  Every result is checked
against a short restatement of SetLookupState + isInKernelExec below, and match / skip also against Arrow C++
(pyarrow.compute.is_in with skip_nulls=False / True)."""
import ctypes
import decimal
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

BEHAVIOURS = ("match", "skip", "emit_null", "inconclusive")
BASE_BINARY = (pa.string(), pa.binary(), pa.large_string(), pa.large_binary())


# ---- no GPU needed ------------------------------------------------------------------------------------------------
def test_is_in_entry_points_are_declared_and_exported():
    from arrow_go_amd import _native as N
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for sym in ("ah_is_in_binary", "ah_is_in_fixed", "ah_is_in_dict_gather"):
        assert sym in N.declared_symbols() and sym in exported, sym


def test_is_in_dispatches_for_byte_string_types():
    """ids as arrow.Type: String 13, Binary 14, FixedSizeBinary 15, Decimal128 23, Decimal256 24, LargeString 34,
    LargeBinary 35; each resolves to itself.  Boolean (1) stays unregistered."""
    from arrow_go_amd import compute as ac
    for tid in (13, 14, 34, 35, 15, 23, 24):
        tin, tout, err = (ctypes.c_int * 1)(tid), (ctypes.c_int * 1)(), ctypes.create_string_buffer(512)
        assert ac.lib.ahc_dispatch_best(b"is_in", 1, tin, tout, err, len(err)) == 0, (tid, err.value)
        assert tout[0] == tid
    tin, tout, err = (ctypes.c_int * 1)(1), (ctypes.c_int * 1)(), ctypes.create_string_buffer(512)
    assert ac.lib.ahc_dispatch_best(b"is_in", 1, tin, tout, err, len(err)) != 0
    assert b"has no kernel matching input types" in err.value


# ---- the restatement --------------------------------------------------------------------------------------------------
def restate(values, value_set, behaviour):
    """SetLookupState.Init (kernels/scalar_set_lookup.go:192-244) + isInKernelExec (:374-413) over Python values"""
    has_null = any(v is None for v in value_set) and behaviour != "skip"
    members = {v for v in value_set if v is not None}
    out = []
    for v in values:
        if v is None:
            out.append((True if has_null else False) if behaviour == "match" else (False if behaviour == "skip" else None))
        elif v in members:
            out.append(True)
        else:
            out.append(None if behaviour == "inconclusive" and has_null else False)
    return out


def _pylist(x):
    if isinstance(x, pa.ChunkedArray):
        return [v for c in x.chunks for v in c.to_pylist()]
    return x.to_pylist()


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.close()


def _is_in(sess, a, vs, behaviour):
    return sess.call_function("is_in", [a], "null_matching_behavior=" + behaviour, value_set=vs)


def _check(sess, a, vs, what="", arrow=True):
    values, vset = _pylist(a), _pylist(vs)
    if isinstance(a, pa.DictionaryArray):
        values = a.cast(a.type.value_type).to_pylist()
    for nb in BEHAVIOURS:
        got = _is_in(sess, a, vs, nb)
        assert _pylist(got) == restate(values, vset, nb), (what, a.type, nb)
    if arrow:
        plain = a.cast(a.type.value_type) if isinstance(a, pa.DictionaryArray) else a
        pvs = pa.concat_arrays(vs.chunks) if isinstance(vs, pa.ChunkedArray) and vs.num_chunks else vs
        if isinstance(pvs, pa.ChunkedArray):
            pvs = pa.array([], vs.type)
        for nb, skip in (("match", False), ("skip", True)):
            assert _pylist(_is_in(sess, a, vs, nb)) == _pylist(pc.is_in(plain, value_set=pvs, skip_nulls=skip)), (what, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("typ", BASE_BINARY, ids=str)
def test_reference_is_in_binary_table(sess, typ):
    """TestIsInBinary (compute/scalar_set_lookup_test.go:180-224), verbatim ("YWFh" = "aaa", "Y2M=" = "cc")"""
    inp = [b"aaa", b"", b"cc", None, b""]
    cases = [
        ([b"aaa", b""], [[True, True, False, False, True], [True, True, False, False, True],
                         [True, True, False, None, True], [True, True, False, None, True]]),
        ([b"aaa", b"", None], [[True, True, False, True, True], [True, True, False, False, True],
                               [True, True, False, None, True], [True, True, None, None, True]]),
        ([None, b"aaa", b"aaa", b"", b"", None], [[True, True, False, True, True], [True, True, False, False, True],
                                                  [True, True, False, None, True], [True, True, None, None, True]]),
    ]
    conv = (lambda v: v if v is None else v.decode()) if typ in (pa.string(), pa.large_string()) else (lambda v: v)
    a = pa.array([conv(v) for v in inp], typ)
    for vs, expected in cases:
        v = pa.array([conv(x) for x in vs], typ)
        for nb, exp in zip(BEHAVIOURS, expected):
            assert _is_in(sess, a, v, nb).to_pylist() == exp, (typ, vs, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 2, 4, 8, 3, 16, 32, 37])
def test_fixed_size_binary_against_restatement(sess, width):
    """TestIsInFixedSizeBinary / …FastPaths: widths 1, 2, 4, 8 take the numeric kernels, others the byte-string table;
    values equal except in their last byte must differ"""
    base = [bytes([i % 7]) * (width - 1) + bytes([i % 5]) for i in range(40)]
    a = pa.array([None if i % 9 == 4 else base[i % len(base)] for i in range(3001)], pa.binary(width))
    for vs in ([base[0], base[3], base[3]], [base[1], None], [], [None]):
        _check(sess, a, pa.array(vs, pa.binary(width)), ("fsb", width))
    _check(sess, a.slice(5, 2003), pa.array(base[2:9], pa.binary(width)).slice(1, 5), ("fsb sliced", width))


@pytest.mark.gpu
@pytest.mark.parametrize("typ", [pa.decimal128(12, 3), pa.decimal256(40, 5)], ids=str)
def test_decimal_against_restatement(sess, typ):
    """TestIsInDecimal, same-type value sets; values one unit apart differ only in their low byte"""
    d = decimal.Decimal
    vals = [d("1.000"), d("1.001"), d("-1.000"), d("0"), d("123456.789")] if typ.precision < 20 else \
        [d("1.00000"), d("1.00001"), d("-1.00000"), d("0"), d("12345678901234567890.12345")]
    a = pa.array([None if i % 7 == 3 else vals[i % len(vals)] for i in range(1000)], typ)
    _check(sess, a, pa.array([vals[0], vals[2]], typ), typ)
    _check(sess, a, pa.array([vals[1], None, vals[1]], typ), typ)


@pytest.mark.gpu
@pytest.mark.parametrize("index_type", [pa.int8(), pa.uint8(), pa.int16(), pa.uint16(), pa.int32(), pa.uint32(), pa.int64(), pa.uint64()], ids=str)
def test_dictionary_equals_decode_then_is_in(sess, index_type):
    """TestIsInDictionary: null indices, a null dictionary entry, unused entries; every index type"""
    dictionary = pa.array(["a", "bb", None, "", "unused", "ccc"], pa.string())
    idx = pa.array([0, 1, None, 2, 3, 5, 0, None, 1, 3] * 37, index_type)
    a = pa.DictionaryArray.from_arrays(idx, dictionary)
    for vs in (["a", ""], ["bb", None], [], [None], ["zz"]):
        _check(sess, a, pa.array(vs, pa.string()), ("dict", index_type), arrow=False)
    num = pa.DictionaryArray.from_arrays(pa.array([0, 1, None, 2, 1], index_type), pa.array([10, None, 30], pa.int64()))
    _check(sess, num, pa.array([10, None], pa.int64()), "numeric dictionary", arrow=False)
    _check(sess, a.slice(3, 200), pa.array(["a", "ccc"], pa.string()), ("dict sliced", index_type), arrow=False)


@pytest.mark.gpu
def test_chunked_input_and_value_set(sess):
    """TestIsInChunked: a chunked value set (empty chunks included) goes into one table, chunk boundaries of the input stay"""
    a = pa.chunked_array([["a", "b", None], [], ["", "c", "a"]], pa.string())
    vs = pa.chunked_array([[], ["a"], [None, ""], []], pa.string())
    _check(sess, a, vs, "chunked")
    got = _is_in(sess, a, vs, "match")
    # the input's boundaries, as numeric is_in keeps them (an empty chunk makes no span in the reference either)
    assert isinstance(got, pa.ChunkedArray) and [len(c) for c in got.chunks] == [3, 3]
    _check(sess, pa.array([1, 2, None, 4], pa.int64()), pa.chunked_array([[1], [None, 4], []], pa.int64()), "numeric chunked set")
    _check(sess, pa.array([1, 2, None, 4], pa.int32()), pa.chunked_array([[1], [4]], pa.int64()), "numeric chunked set, cast")
    _check(sess, pa.array(["a"], pa.string()), pa.chunked_array([], pa.string()), "no chunks")


def _random_strings(rng, n, pool):
    lens = rng.integers(0, 24, size=pool)
    words = [bytes(rng.integers(97, 101, size=l, dtype=np.uint8)) for l in lens]
    pick = rng.integers(0, pool, size=n)
    nulls = rng.random(n) < 0.1
    return [None if nulls[i] else words[pick[i]] for i in range(n)], words


@pytest.mark.gpu
@pytest.mark.parametrize("set_size", [0, 1, 1000, 100_000])
def test_random_columns_every_tier(sess, set_size):
    """2^20 rows, ~10 % nulls, sliced at odd offsets on both sides; value sets of 0 / 1 / 1000 / 100 000 entries (LDS, big LDS
    and HBM tiers), with nulls and duplicates"""
    rng = np.random.default_rng(set_size + 7)
    vals, words = _random_strings(rng, 1 << 20, 4000)
    for typ in (pa.binary(), pa.large_string()):
        conv = (lambda v: v if v is None else v.decode()) if typ == pa.large_string() else (lambda v: v)
        a = pa.array([conv(v) for v in vals], typ).slice(3, (1 << 20) - 10)
        setv = [conv(words[i]) for i in rng.integers(0, 8000, size=set_size) if i < len(words)]
        setv += [conv(b"x%dy" % i) for i in range(set_size - len(setv))]
        if set_size > 1:
            setv[5] = None
        v = pa.array(setv + setv[:3], typ).slice(1) if set_size else pa.array([], typ)
        _check(sess, a, v, ("random", typ, set_size))
    # the 4096-entry big-LDS tier, FixedSizeBinary
    fsb = pa.array([None if i % 10 == 0 else (b"%011d" % (i % 9000)) for i in range(200_001)], pa.binary(11)).slice(1)
    _check(sess, fsb, pa.array([b"%011d" % i for i in range(0, 8000, 2)], pa.binary(11)), "fsb 4000")


@pytest.mark.gpu
def test_edge_cases(sess):
    long = b"q" * 5000
    a = pa.array([b"", b"a", long, long[:-1] + b"r", b"ab\x00", b"ab", None, long + b"\x00", b"z"] * 100, pa.binary())
    for vs in ([long], [b"", None], [b"ab"], [b"ab\x00"], [None, None], [long[:-1] + b"r", b"z"]):
        _check(sess, a, pa.array(vs, pa.binary()), ("edge", vs[:1]))
    _check(sess, pa.array([], pa.string()), pa.array(["a"], pa.string()), "empty input")
    # many long values in one wave next to short ones: the wave-cooperative compare
    rng = np.random.default_rng(3)
    longs = [bytes(rng.integers(0, 256, size=4096 + i, dtype=np.uint8)) for i in range(50)]
    col = pa.array([longs[i % 50] if i % 3 == 0 else bytes([i % 256]) for i in range(20_000)], pa.large_binary())
    _check(sess, col, pa.array(longs[::2] + [bytes([7])], pa.large_binary()), "long values")
    # two strings that differ only in the last byte of a long common prefix
    _check(sess, pa.array([long[:-1] + b"s", long], pa.binary()), pa.array([long[:-1] + b"t"], pa.binary()), "last byte")


@pytest.mark.gpu
def test_mixed_value_set_types(sess):
    from arrow_go_amd.compute import ArrowError
    a = pa.array(["a", "b", None], pa.string())
    assert _is_in(sess, a, pa.array(["a"], pa.large_string()), "match").to_pylist() == [True, False, False]
    assert _is_in(sess, pa.array([b"a"], pa.large_binary()), pa.array([b"a"], pa.binary()), "match").to_pylist() == [True]
    refused = [
        (a, pa.array([b"a"], pa.binary()), "not implemented"),
        (pa.array([b"a"], pa.large_binary()), pa.array(["a"], pa.string()), "not implemented"),
        (pa.array([decimal.Decimal("1.0")], pa.decimal128(5, 1)), pa.array([decimal.Decimal("1.00")], pa.decimal128(5, 2)), "not implemented"),
        (pa.array([b"ab"], pa.binary(2)), pa.array([b"abc"], pa.binary(3)), "not implemented"),
        (a, pa.array([1], pa.int64()), "array type doesn't match type of values set"),
    ]
    for col, vs, msg in refused:
        with pytest.raises(ArrowError) as e:
            _is_in(sess, col, vs, "match")
        assert msg in str(e.value).lower() or msg in str(e.value), (col.type, vs.type, str(e.value))
