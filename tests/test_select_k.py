"""select_k: the first k entries of sort_indices without the sort (csrc/ah_select.hip, kernels.cc SelectKImpl).

The contract is one sentence: select_k(keys, k) == sort_indices(keys)[:min(k, n)].  The stable sort has one answer, so every test
compares the index vector itself, as lists, with Arrow C++'s stable array_sort_indices / sort_indices cut at k.  Every case runs on
the radix route (select_k_route = 1) and on the sort route (2) and must give the same list; a subset also runs with the automatic
choice (0).

Sizes the kernels care about (ah_select.hip): 1024 rows = one workgroup iteration of the classify and histogram passes and one
wave's share of a tile; 4096 rows = kSelTile, the tile of the count / fill passes; 2048 pairs = kSelRankSort, above which the
survivors are ordered by LSD passes (whose own tile is 2048 pairs) instead of the one-workgroup bitonic network; 1024 rows = kSelSmallBin,
the surviving bin at which the threshold levels stop early."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = (1, 2)
NUMERIC = [pa.int8(), pa.uint8(), pa.int16(), pa.uint16(), pa.int32(), pa.uint32(), pa.int64(), pa.uint64(), pa.float32(), pa.float64()]
ORDERS = [(o, p) for o in ("ascending", "descending") for p in ("at_end", "at_start")]


# ---- without a GPU --------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    from arrow_go_amd import _native as N
    assert "ah_select_k" in N.declared_symbols()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "arrowhip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ah_select_k\s*\(\s*ah_ctx\s*\*", header)
    for name, value in (("AH_SELECT_AUTO", 0), ("AH_SELECT_RADIX", 1), ("AH_SELECT_SORT", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    assert any(l.split()[-1] == "ah_select_k" and " T " in l for l in out.splitlines())
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "ah_select_k")


def test_both_names_are_registered_with_one_set_of_kernels():
    from arrow_go_amd import compute as ac
    assert ac.has_function("select_k") and ac.has_function("select_k_unstable")
    assert ac.function_num_kernels("select_k") == ac.function_num_kernels("select_k_unstable") >= 0


def test_the_wrapper_writes_the_option_string():
    """what Session.select_k sends; a k that cannot be written is refused before anything is sent.  The refusals of the library
    itself (k missing, k = -1, more than 8 keys, a column that does not exist) need a session: they are checked in
    test_option_string_errors_from_the_library"""
    from arrow_go_amd import compute as ac
    assert ac.select_k_options(7) == "k=7;order=ascending;null_placement=at_end"
    assert ac.select_k_options(0, order="descending", null_placement="at_start") == "k=0;order=descending;null_placement=at_start"
    assert ac.select_k_options(3, [(1, "desc", "at_start"), (0, "ascending"), 2]) == "k=3;sort_keys=1:desc:at_start,0:asc:at_end,2:asc:at_end"
    for bad in (None, -1, 2.5, True):
        with pytest.raises(ValueError, match="k must be an integer >= 0"):
            ac.select_k_options(bad)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.set_option("select_k_route", 0)
    s.close()


def sorted_rows(values, order="ascending", null_placement="at_end", sort_keys=None):
    """the whole stable sort order, by Arrow C++"""
    if sort_keys is None:
        return pc.array_sort_indices(values, order=order, null_placement=null_placement).to_pylist()
    names = values.schema.names
    return pc.sort_indices(values, sort_keys=[(names[c], "descending" if o == "desc" else "ascending") for c, o, _ in sort_keys],
                           null_placement=sort_keys[0][2]).to_pylist()


def check(sess, values, ks, order="ascending", null_placement="at_end", sort_keys=None, routes=ROUTES, want=None):
    """select_k on every route for every k against the head of the sort order (computed once)"""
    full = want if want is not None else sorted_rows(values, order, null_placement, sort_keys)
    n = len(full)
    for k in ks:
        if k < 0:
            continue
        exp = full[:min(k, n)]
        for route in routes:
            sess.set_option("select_k_route", route)
            got = sess.select_k(values, k, sort_keys=sort_keys, order=order, null_placement=null_placement)
            assert got.type == pa.uint64() and got.null_count == 0
            assert got.to_pylist() == exp, (n, k, order, null_placement, sort_keys, route)


def ks_for(n, extra=()):
    return sorted(set([0, 1, 2, n // 2, n - 1, n, n + 5] + list(extra)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8193, 70001])
def test_sizes(sess, n):
    """Int32 with a tenth nulls; k at both ends, in the middle and on both sides of the bitonic network's 2048 pairs"""
    rng = np.random.default_rng(n)
    a = pa.array(rng.integers(-10**6, 10**6, n).astype(np.int32), mask=rng.random(n) < 0.1)
    ks = ks_for(n, [k for k in (1000, 2047, 2048, 2049, 3100) if k < n])
    check(sess, a, ks, routes=(0, 1, 2) if n in (65, 4097, 70001) else ROUTES)
    check(sess, a, [1, n // 3, n], "descending", "at_start")


@pytest.mark.gpu
@pytest.mark.parametrize("typ", NUMERIC, ids=str)
def test_every_numeric_type_both_orders_both_placements(sess, typ):
    rng = np.random.default_rng(typ.bit_width + 7 * pa.types.is_signed_integer(typ) + 3 * pa.types.is_floating(typ))
    n = 5003
    if pa.types.is_floating(typ):
        vals = rng.normal(0, 1e3, n).astype(typ.to_pandas_dtype())
        vals[rng.random(n) < 0.05] = np.nan
    elif typ == pa.uint64():
        vals = rng.integers(0, 2**64, n, dtype=np.uint64)          # half of them above 2^63
        vals[:5] = [2**64 - 1, 2**63, 2**63 - 1, 0, 2**63 + 1]
    else:
        info = np.iinfo(typ.to_pandas_dtype())
        vals = rng.integers(info.min, int(info.max) + 1, n, dtype=typ.to_pandas_dtype())   # Int8 / UInt8: 256 values, ties everywhere
    a = pa.array(vals, mask=rng.random(n) < 0.1, type=typ).slice(5, n - 9)
    for order, npl in ORDERS:
        check(sess, a, [1, 40, 700, 2600, len(a) - 1], order, npl)


@pytest.mark.gpu
def test_ties_across_tiles(sess):
    n = 70001
    const = pa.array(np.full(n, 42, np.int64))
    for route in (0, 1, 2):
        sess.set_option("select_k_route", route)
        assert sess.select_k(const, 35000).to_pylist() == list(range(35000))      # a constant column: the first k rows
    check(sess, const, [1, 4097, n], "descending")
    rng = np.random.default_rng(5)
    two = pa.array(np.where(rng.random(n) < 0.5, 7, -7).astype(np.int32))              # two distinct values
    check(sess, two, [1, 3000, 35000, 60000])
    check(sess, two, [3000, 35000], "descending")
    # the threshold value sits in rows spread over ≥ 3 tiles of 4096 rows, and more of them exist than are needed
    v = rng.integers(1000, 10**6, 20000).astype(np.int64)
    v[:50] = rng.integers(0, 100, 50)                # 50 rows below the threshold value 500
    tie_rows = np.array([100, 3000, 4095, 4096, 4097, 9000, 12287, 12288, 15000, 19999])
    v[tie_rows] = 500
    a = pa.array(v)
    want = sorted_rows(a)
    assert sorted(want[50:60]) == tie_rows.tolist()
    check(sess, a, [50, 51, 53, 57, 59, 60, 61], want=want)


@pytest.mark.gpu
def test_level_logic(sess):
    rng = np.random.default_rng(11)
    n = 9001
    base = np.int64(0x1234_5678_9ABC_DE00)
    low3 = pa.array(base + rng.integers(0, 8, n).astype(np.int64))                     # keys that differ only in their lowest 3 bits
    top = pa.array((rng.integers(-8, 8, n).astype(np.int64) << 60) + 5)                # … only in the top bits
    ends = pa.array(rng.choice(np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, 0], np.int64), n))
    small = pa.array(rng.integers(0, 10**5, n).astype(np.int64))                       # the normalised first level
    spread = pa.array(rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n, dtype=np.int64))   # all six levels' worth of bits
    for a in (low3, top, ends, small, spread):
        for order in ("ascending", "descending"):
            check(sess, a, [1, 17, 1500, 4500, n - 1], order)
    # a bin that stays above kSelSmallBin rows for several levels: 6000 keys that share their upper 40 bits
    v = rng.integers(0, 2**62, 20000).astype(np.int64)
    v[rng.choice(20000, 6000, replace=False)] = (np.int64(3) << 40) + rng.integers(0, 2**20, 6000)
    check(sess, pa.array(v), [1, 100, 1024, 1025, 3000, 5999, 6000, 6001])


@pytest.mark.gpu
@pytest.mark.parametrize("typ", [pa.float32(), pa.float64()], ids=str)
def test_floats(sess, typ):
    rng = np.random.default_rng(13)
    dt = typ.to_pandas_dtype()
    tiny = np.finfo(dt).tiny
    pool = np.array([0.0, -0.0, np.inf, -np.inf, tiny / 4, -tiny / 4, tiny / 2, 1.5, -1.5, np.nan], dt)   # ±0, ±inf, denormals, NaN
    n = 6000
    vals = rng.choice(pool, n)
    a = pa.array(vals, mask=rng.random(n) < 0.2, type=typ).slice(3)
    want_n = len(a)
    n_null, n_nan = a.null_count, int(np.isnan(a.drop_null().to_numpy()).sum())
    n_rest = want_n - n_null - n_nan
    for order, npl in ORDERS:
        inside_nan = n_rest + n_nan // 2 if npl == "at_end" else n_null + n_nan // 2
        inside_null = n_rest + n_nan + n_null // 2 if npl == "at_end" else n_null // 2
        check(sess, a, [1, 700, n_rest, inside_nan, inside_null, want_n], order, npl)
    zeros = pa.array(rng.choice(np.array([0.0, -0.0], dt), 5000), type=typ)             # −0.0 ties +0.0: the first k rows
    check(sess, zeros, [1, 2500, 4999], want=list(range(5000)))
    check(sess, zeros, [2500], "descending", want=list(range(5000)))
    all_nan = pa.array(np.full(4100, np.nan, dt), type=typ)
    all_null = pa.array([None] * 4100, type=typ)
    for order, npl in ORDERS:
        check(sess, all_nan, [1, 4097, 4100], order, npl, want=list(range(4100)))
        check(sess, all_null, [1, 4097, 4105], order, npl, want=list(range(4100)))


@pytest.mark.gpu
def test_validity_offsets_and_more_nulls_than_k(sess):
    rng = np.random.default_rng(17)
    n = 9000
    whole = pa.array(rng.integers(-500, 500, n).astype(np.int16), mask=rng.random(n) < 0.3)
    for off in range(8):
        a = whole.slice(off, n - 2 * off - 1)
        check(sess, a, [1, 800, 5000], "ascending", "at_end" if off % 2 else "at_start")
    mostly_null = pa.array(rng.integers(0, 9, n).astype(np.int64), mask=rng.random(n) < 0.9).slice(2)
    want = sorted_rows(mostly_null, "ascending", "at_start")
    null_rows = [i for i, v in enumerate(mostly_null.to_pylist()) if v is None]
    assert want[:4200] == null_rows[:4200]                       # the answer is the first k null rows
    check(sess, mostly_null, [1, 4097, 4200], "ascending", "at_start", want=want)
    check(sess, mostly_null, [len(null_rows) + 3], "descending", "at_start")


@pytest.mark.gpu
def test_several_keys(sess):
    rng = np.random.default_rng(19)
    n = 30011
    i32 = pa.array(rng.integers(0, 200, n).astype(np.int32), mask=rng.random(n) < 0.02)
    f64 = rng.normal(0, 1, n)
    f64[rng.random(n) < 0.03] = np.nan
    f64 = pa.array(f64, mask=rng.random(n) < 0.05)
    i64 = pa.array(rng.integers(-10**12, 10**12, n).astype(np.int64))
    batch = pa.record_batch([i32, f64, i64], names=["a", "b", "c"])
    # (Int32, Float64): about 150 rows per key-0 value, so the tie range on key 0 straddles every k
    check(sess, batch, [1, 75, 1000, 3500, 3501, n - 1], sort_keys=[(0, "asc", "at_end"), (1, "asc", "at_end")], routes=(0, 1, 2))
    check(sess, batch, [100, 29000, n + 5], sort_keys=[(0, "desc", "at_end"), (1, "desc", "at_end"), (2, "asc", "at_end")])
    # (Float64 desc at_start, Int64 asc): nulls and NaNs of key 0 come first, so small k are answered inside those groups
    check(sess, batch, [1, 1000, 2500, 5000], sort_keys=[(1, "desc", "at_start"), (2, "asc", "at_start")])
    # few candidates: key 0 almost unique, the second key decides inside pairs of equal keys
    pairs = pa.record_batch([pa.array((rng.permutation(n) // 2).astype(np.int64)), i64], names=["a", "c"])
    check(sess, pairs, [1, 2, 3, 999, 1000, 5001], sort_keys=[(0, "asc", "at_end"), (1, "desc", "at_end")])
    # the columns of the batch as separate arguments
    sess.set_option("select_k_route", 1)
    got = sess.call_function("select_k", [i32, f64], "k=500;sort_keys=0:asc:at_end,1:asc:at_end").to_pylist()
    assert got == sorted_rows(batch, sort_keys=[(0, "asc", "at_end"), (1, "asc", "at_end")])[:500]
    assert sess.call_function("select_k_unstable", [i32, f64], "k=500;sort_keys=0:asc:at_end,1:asc:at_end").to_pylist() == got


@pytest.mark.gpu
def test_string_keys_take_the_sort_route(sess):
    from arrow_go_amd import compute as ac
    rng = np.random.default_rng(23)
    n = 5000
    s = pa.array(["k%03d" % i for i in rng.integers(0, 300, n)], mask=rng.random(n) < 0.1)
    i32 = pa.array(rng.integers(0, 40, n).astype(np.int32))
    check(sess, s, [1, 100, n], routes=(0, 2))                                          # a string first key
    sess.set_option("select_k_route", 1)
    with pytest.raises(ac.ErrNotImplemented, match="numeric first key"):                # forcing the radix route never gives a wrong answer
        sess.select_k(s, 10)
    batch = pa.record_batch([s, i32], names=["s", "i"])
    check(sess, batch, [1, 700], sort_keys=[(0, "asc", "at_end"), (1, "desc", "at_end")], routes=(0, 2))
    check(sess, batch, [1, 700, 2600], sort_keys=[(1, "asc", "at_end"), (0, "desc", "at_end")])   # a string second key


@pytest.mark.gpu
def test_chunked_temporal_and_take(sess):
    rng = np.random.default_rng(29)
    vals = rng.integers(0, 10**4, 20000).astype(np.int64)
    whole = pa.array(vals, mask=rng.random(20000) < 0.1)
    chunked = pa.chunked_array([whole.slice(0, 7), whole.slice(7, 9000), whole.slice(9007, 1), whole.slice(9008)])   # uneven chunks
    check(sess, chunked, [1, 5000, 20005], "descending", "at_start", want=sorted_rows(whole, "descending", "at_start"))
    ts = pa.array(vals * 1000, mask=rng.random(20000) < 0.1).cast(pa.timestamp("us"))
    d32 = pa.array((vals % 3000).astype(np.int32)).cast(pa.date32())
    check(sess, ts, [1, 3000], "descending")
    check(sess, d32, [1, 3000, 9000])
    # take(batch, select_k(...)) == the head of sort
    batch = pa.record_batch([whole, pa.array(rng.integers(0, 100, 20000).astype(np.int32))], names=["a", "b"])
    keys = [(1, "asc", "at_end"), (0, "desc", "at_end")]
    for route in ROUTES:
        sess.set_option("select_k_route", route)
        idx = sess.select_k(batch, 1234, sort_keys=keys)
        head = sess.call_function("take", [batch, idx])
        assert head.equals(sess.call_function("sort", [batch], "sort_keys=1:asc:at_end,0:desc:at_end").slice(0, 1234))


@pytest.mark.gpu
def test_option_string_errors_from_the_library(sess):
    from arrow_go_amd import compute as ac
    a = pa.array([3, 1, 2], pa.int32())
    b = pa.array([1.0, 2.0, 3.0])
    sess.set_option("select_k_route", 0)
    with pytest.raises(ac.ErrInvalid, match="non-negative k"):
        sess.call_function("select_k", [a], "order=ascending")                         # k missing
    with pytest.raises(ac.ErrInvalid, match="non-negative k"):
        sess.call_function("select_k", [a], "k=-1;order=ascending")                    # k = -1
    with pytest.raises(ac.ErrInvalid, match="non-negative k"):
        sess.call_function("select_k", [a], "k=two")
    with pytest.raises(ac.ErrNotImplemented, match="more than 8 sort keys"):
        sess.call_function("select_k", [a, b], "k=1;sort_keys=" + ",".join("%d:asc:at_end" % (i % 2) for i in range(9)))
    with pytest.raises(ac.ErrInvalid, match="invalid column index"):
        sess.call_function("select_k", [a, b], "k=1;sort_keys=0:asc:at_end,2:asc:at_end")   # a column that does not exist
    with pytest.raises(ac.ErrInvalid, match="select_k_route"):
        sess.set_option("select_k_route", 3)
    assert sess.call_function("select_k", [a], "k=2").to_pylist() == [1, 2]             # the keys default to one ascending key
    assert sess.call_function("select_k", [a], "k=0;order=descending").to_pylist() == []
