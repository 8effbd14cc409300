"""sort_indices / sort by String, Binary, LargeString, LargeBinary, FixedSizeBinary and Decimal128 / 256 keys
(arrow/compute/internal/kernels/vector_sort.go:195-245), alone and mixed with numeric keys.  A stable sort has exactly one
answer, so every check compares the permutation itself; Arrow C++ (pyarrow.compute.sort_indices) orders these types the same
way — bytewise, unsigned, a proper prefix first; decimals by value — and serves as the independent cross-check."""
import ctypes
import decimal
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = [(o, p) for o in ("ascending", "descending") for p in ("at_end", "at_start")]


# ---- no GPU needed ------------------------------------------------------------------------------------------------
def test_sort_indices_keys_is_declared_and_exported():
    from arrow_go_amd import _native as N
    from arrow_go_amd import compute as ac
    assert "ah_sort_indices_keys" in N.declared_symbols()
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    assert "ah_sort_indices_keys" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert ac.has_function("sort_indices") and ac.has_function("sort")


def test_sort_key_ids_follow_arrow_type(tmp_path):
    """the key ids are arrow.Type values (arrow/datatype.go): BINARY 14, FIXED_SIZE_BINARY 15, DECIMAL128 23, DECIMAL256 24,
    LARGE_BINARY 35; the descriptor is plain C"""
    src = ('#include "arrowhip.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%d %d %d %d %d %d", AH_BINARY, '
           'AH_FIXED_SIZE_BINARY, AH_DECIMAL128, AH_DECIMAL256, AH_LARGE_BINARY, (int)sizeof(ah_sort_key)); return 0; }\n')
    exe = str(tmp_path / "sort_key_ids")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src, text=True, check=True)
    ids = [int(v) for v in subprocess.check_output([exe], text=True).split()]
    assert ids[:5] == [pa.binary().id, pa.binary(4).id, pa.decimal128(5, 0).id, pa.decimal256(5, 0).id, pa.large_binary().id]
    assert ids[5] == 56 if ctypes.sizeof(ctypes.c_void_p) == 8 else True


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.close()


def _si(sess, a, order="ascending", npl="at_end"):
    return sess.call_function("sort_indices", [a], "order=%s;null_placement=%s" % (order, npl)).to_pylist()


def _check_all_orders(sess, a, what=""):
    for order, npl in ORDERS:
        exp = pc.array_sort_indices(a, order=order, null_placement=npl).to_pylist()
        assert _si(sess, a, order, npl) == exp, (what, a.type, order, npl)


def _validity(mask):
    return pa.array(~mask).buffers()[1]


def _var_values(rng, n, maxlen=12, alphabet=b"ab\x00c\xff"):
    lens = rng.integers(0, maxlen + 1, n)
    pool = np.frombuffer(alphabet, np.uint8)
    data = pool[rng.integers(0, len(pool), int(lens.sum()))].tobytes()
    offs = np.concatenate([[0], np.cumsum(lens)])
    return [data[offs[i]:offs[i + 1]] for i in range(n)]


def _make(typ, rng, n):
    """n values of `typ` with ~10 % nulls and plenty of ties"""
    mask = rng.random(n) < 0.1
    if pa.types.is_fixed_size_binary(typ):
        w = typ.byte_width
        pool = np.array([0, 1, 0x7F, 0x80, 0xFF], np.uint8)
        raw = pool[rng.integers(0, len(pool), n * w)]
        if w > 2:  # most rows share all but their last two bytes: ties carry into the later rounds
            raw.reshape(n, w)[:, :w - 2] = raw.reshape(n, w)[rng.integers(0, 3, n), :w - 2] if n else 0
        return pa.Array.from_buffers(typ, n, [_validity(mask), pa.py_buffer(raw.tobytes())])
    if pa.types.is_decimal(typ):
        words = typ.bit_width // 64
        w = np.empty((n, words), np.uint64)
        w[:, 0] = rng.choice(np.array([0, 1, 5, 2**63, 2**64 - 1], np.uint64), n)
        for k in range(1, words):
            w[:, k] = rng.choice(np.array([0, 7, 2**63, 2**64 - 1], np.uint64), n)  # 2^64-1 on top: negative values
        return pa.Array.from_buffers(typ, n, [_validity(mask), pa.py_buffer(w.tobytes())])
    vals = _var_values(rng, n)
    if pa.types.is_string(typ) or pa.types.is_large_string(typ):
        vals = [v.replace(b"\xff", b"z").decode() for v in vals]
    return pa.array(vals, type=typ, mask=mask)


VAR_TYPES = [pa.string(), pa.binary(), pa.large_string(), pa.large_binary()]
FIXED_TYPES = [pa.binary(1), pa.binary(7), pa.binary(8), pa.binary(16), pa.binary(33), pa.decimal128(38, 0), pa.decimal256(76, 0)]


@pytest.mark.gpu
def test_reference_tables(sess):
    # TestSortIndices "StringAscending" :106 and "Binary" :197
    assert _si(sess, pa.array(["cherry", "apple", "banana", "date"])) == [1, 2, 0, 3]
    assert _si(sess, pa.array([b"\x03\x02\x01", b"\x01\x02\x03", b"\x02\x02\x02"], pa.binary())) == [1, 2, 0]
    # TestSortArray "StringAscending" :438 / "Binary" :521: sort = take(input, sort_indices(input))
    assert sess.call_function("sort", [pa.array(["cherry", "apple", "banana", "date"])], "order=ascending").to_pylist() == \
        ["apple", "banana", "cherry", "date"]
    assert sess.call_function("sort", [pa.array([b"\x03\x02\x01", b"\x01\x02\x03", b"\x02\x02\x02"])], "order=ascending").to_pylist() == \
        [b"\x01\x02\x03", b"\x02\x02\x02", b"\x03\x02\x01"]
    # TestSortRecordBatch :554 (category string, value, priority)
    si = lambda cols, keys: sess.call_function("sort_indices", cols, "sort_keys=" + keys).to_pylist()
    I32 = lambda v: pa.array(v, pa.int32())
    assert si([pa.array(["A", "B", "C"]), I32([30, 10, 20]), I32([1, 2, 3])], "1:asc:at_end") == [1, 2, 0]       # SortBySecondColumn :567
    cat, f2, f3 = pa.array(["B", "A", "B", "A"]), I32([1, 1, 2, 2]), I32([100, 200, 300, 400])                 # MultiColumnLexicographic :612
    assert si([cat, f2, f3], "1:asc:at_end,2:desc:at_start") == [1, 0, 3, 2]
    assert si([cat, f2, f3], "0:asc:at_end,1:asc:at_end") == [1, 3, 0, 2]
    # TestSortTable :702 (name string, age): by age; then category / priority / id
    assert si([pa.array(["Alice", "Bob", "Charlie"]), I32([30, 25, 35])], "1:asc:at_end") == [1, 0, 2]
    cat, pri, ids = pa.array(["A", "B", "A", "B"]), I32([2, 1, 1, 2]), I32([100, 200, 300, 400])               # MultiColumnSort :759
    assert si([cat, pri, ids], "1:asc:at_end,2:desc:at_start") == [2, 1, 3, 0]
    assert si([cat, pri, ids], "0:asc:at_end,1:desc:at_end") == [0, 2, 3, 1]
    # TestSortIndicesUUIDLexicographic :1786: a 16-byte fixed-size binary column with a null
    u = pa.array([bytes(15) + b"\x03", None, bytes(15) + b"\x01", bytes(15) + b"\x02"], pa.binary(16))
    assert [_si(sess, u, o, p) for o, p in ORDERS] == [[2, 3, 0, 1], [1, 2, 3, 0], [0, 3, 2, 1], [1, 0, 3, 2]]


@pytest.mark.gpu
def test_order_contract(sess):
    """bytewise, unsigned; a proper prefix first; "ab" < "ab\\0"; empty values first; decimals by signed value"""
    v = [b"abc", b"ab\x00", b"", b"ab", None, b"\xff", b"ab\x00\x00", b"a", b"ab", b"\x7f", b""]
    a = pa.array(v, pa.binary())
    assert _si(sess, a) == [2, 10, 7, 3, 8, 1, 6, 0, 9, 5, 4]
    assert _si(sess, a, "descending", "at_start") == [4, 5, 9, 0, 6, 1, 3, 8, 7, 2, 10]
    _check_all_orders(sess, a)
    _check_all_orders(sess, pa.array([x.decode("latin-1") if x is not None else None for x in v], pa.large_string()))
    d = pa.array([None] + [decimal.Decimal(x) for x in ("-1", "0", "1", "-99999999999999999999999999999999999999",
                                                                       "99999999999999999999999999999999999999", "-18446744073709551616",
                                                                       "18446744073709551616", "-1", "2")], pa.decimal128(38, 0))
    assert _si(sess, d) == [4, 6, 1, 8, 2, 3, 9, 7, 5, 0]
    _check_all_orders(sess, d)
    _check_all_orders(sess, d.cast(pa.decimal256(76, 0)))
    # descending keeps ties in input order
    assert _si(sess, pa.array(["x", "y", "x", "y"]), "descending") == [1, 3, 0, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("typ", VAR_TYPES + FIXED_TYPES, ids=str)
@pytest.mark.parametrize("n", [0, 1, 2, 37, 4099, (1 << 20) + 5])
def test_random_vs_arrow_cpp(sess, typ, n):
    rng = np.random.default_rng(n + typ.id * 7 + (typ.bit_width if pa.types.is_fixed_size_binary(typ) else 0))
    a = _make(typ, rng, n + 3)
    for off in (0, 3):
        _check_all_orders(sess, a.slice(off, n), off)


def _url_like(rng, n):
    host = "https://www.example-cdn-host.com/assets/static/v2/images/products/catalogue/"  # 80 shared bytes
    sub = ["thumbs/", "large/", "large/x/"]
    return [host + sub[rng.integers(0, 3)] + "item-%d.png" % rng.integers(0, n // 4 + 1) for _ in range(n)]


@pytest.mark.gpu
def test_long_common_prefixes(sess):
    rng = np.random.default_rng(5)
    vals = _url_like(rng, 60000)
    mask = rng.random(len(vals)) < 0.1
    for typ in (pa.string(), pa.large_binary()):
        _check_all_orders(sess, pa.array(vals, typ, mask=mask).slice(3), "urls")


@pytest.mark.gpu
def test_many_duplicates_of_long_values(sess):
    """the worst case: every row stays tied round after round (300-byte values differing only at the end)"""
    rng = np.random.default_rng(6)
    base = "q" * 297
    vals = [base + s for s in rng.choice(["aaa", "aab", "aa", "aaa\0"], 20000)]
    _check_all_orders(sess, pa.array(vals, pa.string()), "dups")
    same = pa.array(["z" * 1000] * 3000 + ["z" * 999] * 5, pa.binary())
    assert _si(sess, same) == list(range(3000, 3005)) + list(range(3000))
    _check_all_orders(sess, same)


@pytest.mark.gpu
def test_one_large_run_and_many_small_ones(sess):
    """after the first round: one run above the one-wave limit (long shared prefix) next to thousands of runs of 2-3 rows"""
    rng = np.random.default_rng(7)
    big = ["commonprefix/" + "%04d" % rng.integers(0, 300) for _ in range(5000)]
    small = ["p%06d/x" % (i // 3) + "abc"[rng.integers(0, 3)] for i in range(30000)]
    vals = big + small
    order = rng.permutation(len(vals))
    a = pa.array([vals[i] for i in order], pa.string())
    _check_all_orders(sess, a, "runs")
    # only small runs
    _check_all_orders(sess, pa.array(small[::-1], pa.binary()), "small")


@pytest.mark.gpu
def test_values_ending_at_the_end_of_the_data_buffer(sess):
    for last in (b"x", b"xyzxyzx", b"abcdefgh", b"0123456789abcde"):
        vals = [b"abcdefgh" * 2, b"abcdefgh", last, b"ab", last]
        data = b"".join(vals)
        offs = np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(np.int32)
        a = pa.Array.from_buffers(pa.binary(), len(vals), [None, pa.py_buffer(offs.tobytes()), pa.py_buffer(data)])
        assert a.to_pylist() == vals
        _check_all_orders(sess, a, last)
        _check_all_orders(sess, a.slice(2), last)
    w = pa.Array.from_buffers(pa.binary(33), 3, [None, pa.py_buffer(bytes(range(99)))])
    _check_all_orders(sess, w, "fsb33")


@pytest.mark.gpu
@pytest.mark.parametrize("npl", ["at_end", "at_start"])
def test_multi_key_string_in_every_position(sess, npl):
    rng = np.random.default_rng(8)
    n = 50021
    s = pa.array(["k%02d" % v for v in rng.integers(0, 40, n)], mask=rng.random(n) < 0.1)
    u = pa.array(_url_like(rng, n), pa.large_string())
    i = pa.array(rng.integers(0, 7, n), mask=rng.random(n) < 0.1, type=pa.int16())
    f = pa.array(rng.integers(0, 5, n).astype(np.float64), mask=rng.random(n) < 0.1)
    d = pa.array(rng.integers(0, 3, n), pa.uint64())
    dec = pa.Array.from_buffers(pa.decimal128(38, 0), n, [None, pa.py_buffer(rng.integers(-2, 2, 2 * n).astype(np.int64).tobytes())])
    tbl = pa.table({"s": s, "u": u, "i": i, "f": f, "d": d, "dec": dec})
    cols = [tbl.column(c).combine_chunks() for c in tbl.column_names]
    names = tbl.column_names
    for keys in ([("s", "ascending"), ("i", "descending"), ("f", "ascending")],
                 [("i", "ascending"), ("s", "descending"), ("d", "ascending")],
                 [("f", "descending"), ("i", "ascending"), ("s", "ascending")],
                 [("dec", "descending"), ("u", "ascending"), ("i", "ascending")],
                 [("i", "ascending"), ("u", "descending")]):
        spec = ",".join("%d:%s:%s" % (names.index(k), o[:3] if o == "ascending" else "desc", npl) for k, o in keys)
        got = sess.call_function("sort_indices", cols, "sort_keys=" + spec).to_pylist()
        exp = pc.sort_indices(tbl, sort_keys=keys, null_placement=npl).to_pylist()
        assert got == exp, keys


@pytest.mark.gpu
def test_chunked_input(sess):
    rng = np.random.default_rng(9)
    chunks = [_make(t, rng, m) for t, m in ((pa.string(), 1000), (pa.string(), 0), (pa.string(), 3001))]
    ca = pa.chunked_array(chunks + [chunks[0].slice(5, 100)], pa.string())
    for order, npl in ORDERS:
        got = sess.call_function("sort_indices", [ca], "order=%s;null_placement=%s" % (order, npl)).to_pylist()
        assert got == pc.array_sort_indices(ca.combine_chunks(), order=order, null_placement=npl).to_pylist(), (order, npl)
    lb = pa.chunked_array([pa.array(_url_like(rng, 700), pa.large_binary()) for _ in range(3)])
    assert sess.call_function("sort_indices", [lb], "order=descending").to_pylist() == \
        pc.array_sort_indices(lb.combine_chunks(), order="descending").to_pylist()


@pytest.mark.gpu
def test_sort_returns_sorted_values(sess):
    rng = np.random.default_rng(10)
    for typ in (pa.string(), pa.large_binary(), pa.binary(7), pa.decimal128(38, 0), pa.decimal256(76, 0)):
        a = _make(typ, rng, 5003).slice(3)
        for order, npl in ORDERS:
            got = sess.call_function("sort", [a], "order=%s;null_placement=%s" % (order, npl))
            exp = pc.take(a, pc.array_sort_indices(a, order=order, null_placement=npl))
            assert got.to_pylist() == exp.to_pylist(), (typ, order, npl)


@pytest.mark.gpu
def test_boolean_still_not_implemented(sess):
    from arrow_go_amd import compute as ac
    with pytest.raises(ac.ErrNotImplemented, match="sorting not supported"):
        sess.call_function("sort_indices", [pa.array([True, False])], "order=ascending")
    with pytest.raises(ac.ErrNotImplemented, match="sorting not supported"):
        sess.call_function("sort_indices", [pa.array(["a", "b"]), pa.array([True, False])], "sort_keys=0:asc:at_end,1:asc:at_end")
