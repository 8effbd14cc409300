"""`window` and `rank` through Session.window / Session.rank against the host model (tests/window_model.py) and Arrow C++'s pc.rank.

Batches of TILE + 1 and 3 S + 17 rows (TILE and kSuper read from ah_window.hip, S = kSuper * TILE); partitions by (int32 with
nulls), by (string, bool) and by nothing; orders by nothing, by (float64 desc, nulls first) and by (string asc, int64 desc); all
seven functions at once.  Every output is compared as bytes (values with zeros under the nulls) plus validity.  The float value
column holds integers, so its exact sums are representable and compared byte for byte like the rest."""
import os
import re
import warnings

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc  # noqa: E402

from tests import window_model as WM  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "arrow_go_amd", "csrc", "ah_window.hip")).read()
TILE = int(re.search(r"constexpr int TILE = (\d+);", _SRC).group(1))
S = int(re.search(r"constexpr int kSuper = (\d+);", _SRC).group(1)) * TILE
ALL = ["row_number", "rank", "dense_rank", ("v", "cumulative_sum"), ("v", "cumulative_min"), ("v", "cumulative_max"), ("v", "cumulative_count"),
       ("f", "cumulative_sum"), ("f", "cumulative_min"), ("w", "cumulative_sum"), ("w", "cumulative_max")]
PARTITIONS = {"int32_with_nulls": ["g"], "string_bool": ["s", "b"], "none": []}
ORDERS = {"none": [], "float64_desc_at_start": [("k", "desc", "at_start")], "string_asc_int64_desc": [("t", "asc", "at_end"), ("i", "desc", "at_end")]}
OUT_TYPES = {"row_number": pa.uint64(), "rank": pa.uint64(), "dense_rank": pa.uint64(), "v_cumulative_sum": pa.int64(), "v_cumulative_min": pa.int16(),
             "v_cumulative_max": pa.int16(), "v_cumulative_count": pa.int64(), "f_cumulative_sum": pa.float64(), "f_cumulative_min": pa.float32(),
             "w_cumulative_sum": pa.uint64(), "w_cumulative_max": pa.uint64()}


@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.close()


def make_batch(n, seed=0):
    rng = np.random.default_rng(seed)
    words = np.array(["", "a", "ab", "abc", "b", "0123456789-long-value", "0123456789-long-valuf"])
    cols = {
        "g": pa.array(rng.integers(0, 50, n).astype(np.int32), mask=rng.random(n) < 0.1),
        "s": pa.array(words[rng.integers(0, 4, n)], mask=rng.random(n) < 0.1),
        "b": pa.array(rng.random(n) < 0.5, mask=rng.random(n) < 0.1),
        "k": pa.array(np.array([np.nan, -0.0, 0.0, 1.0, 2.0, 3.5, -4.0])[rng.integers(0, 7, n)], mask=rng.random(n) < 0.1),
        "t": pa.array(words[rng.integers(0, len(words), n)], mask=rng.random(n) < 0.1),
        "i": pa.array(rng.integers(-3, 3, n).astype(np.int64) * (1 << 40), mask=rng.random(n) < 0.1),
        "v": pa.array(rng.integers(-2**15, 2**15, n).astype(np.int16), mask=rng.random(n) < 0.1),
        "f": pa.array(rng.integers(-100, 100, n).astype(np.float32), mask=rng.random(n) < 0.1),   # integers: exact sums
        "w": pa.array(rng.integers(0, 2**64, n, dtype=np.uint64)),   # no nulls: sums wrap
    }
    return pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols))


def same(got, want):
    """got: the library's record batch; want: the model's dict"""
    assert got.schema.names == list(want)
    for name, (values, valid) in want.items():
        col = got.column(got.schema.names.index(name))
        assert col.type == OUT_TYPES[name], name
        if isinstance(values, list):
            values = np.array([float(f) for f in values], np.float64)
        if valid is None:
            assert col.null_count == 0, name
        else:
            assert col.is_valid().to_pylist() == valid.tolist(), name
        have = col.fill_null(0).to_numpy(zero_copy_only=False) if col.null_count else col.to_numpy(zero_copy_only=False)
        assert have.dtype == values.dtype and have.tobytes() == values.tobytes(), name


@pytest.fixture(scope="module")
def batches():
    return {n: make_batch(n, seed=n) for n in (TILE + 1, 3 * S + 17)}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("partition", list(PARTITIONS))
@pytest.mark.parametrize("n", [TILE + 1, 3 * S + 17], ids=["tile_plus_1", "3S_plus_17"])
def test_all_functions_against_the_model(sess, batches, n, partition, order):
    batch = batches[n]
    got = sess.window(batch, PARTITIONS[partition], ORDERS[order], ALL)
    assert got.num_rows == n
    same(got, WM.window(batch, PARTITIONS[partition], ORDERS[order], ALL))


def test_float_min_max_through_the_api(sess):
    n = TILE + 1
    rng = np.random.default_rng(4)
    pool = np.array([np.nan, -0.0, 0.0, 1.0, 2.5, -7.0, np.inf, -np.inf], np.float64)
    batch = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 200, n).astype(np.int8)), pa.array(pool[rng.integers(0, len(pool), n)], mask=rng.random(n) < 0.2)],
                                       names=["g", "x"])
    fns = [("x", "cumulative_min"), ("x", "cumulative_max"), ("x", "cumulative_count")]
    got, want = sess.window(batch, ["g"], [], fns), WM.window(batch, ["g"], [], fns)
    for name, (values, valid) in want.items():
        col = got.column(got.schema.names.index(name))
        assert col.fill_null(0).to_numpy(zero_copy_only=False).tobytes() == values.tobytes(), name
        assert valid is None or col.is_valid().to_pylist() == valid.tolist()


@pytest.mark.parametrize("off", [3, 69])
def test_sliced_batches(sess, batches, off):
    whole = batches[TILE + 1]
    batch = whole.slice(off, TILE + 1 - off - 5)
    for partition, order in (("int32_with_nulls", "float64_desc_at_start"), ("string_bool", "string_asc_int64_desc"), ("none", "none")):
        got = sess.window(batch, PARTITIONS[partition], ORDERS[order], ALL)
        same(got, WM.window(batch, PARTITIONS[partition], ORDERS[order], ALL))


@pytest.mark.parametrize("n", [0, 1])
def test_tiny_batches(sess, n):
    batch = make_batch(8, seed=1).slice(2, n)
    got = sess.window(batch, ["g"], ORDERS["float64_desc_at_start"], ALL)
    assert got.num_rows == n and got.schema.names == list(OUT_TYPES)
    assert [c.type for c in got.columns] == list(OUT_TYPES.values())
    if n:
        same(got, WM.window(batch, ["g"], ORDERS["float64_desc_at_start"], ALL))
    got = sess.window(batch, [], [], ["row_number"])
    assert got.column(0).to_pylist() == [1] * n


def test_a_table_of_single_chunks_is_taken(sess):
    batch = make_batch(100, seed=2)
    got = sess.window(pa.Table.from_batches([batch]), ["g"], [], ["row_number"])
    assert got.equals(sess.window(batch, ["g"], [], ["row_number"]))


def test_keep_on_device_chains_into_take(sess):
    """rank stays in HBM and is gathered there: take(rank(v), sort_indices(v)) is the ranks in sort order, so non-decreasing"""
    rng = np.random.default_rng(8)
    v = pa.array(rng.integers(0, 50, TILE + 1).astype(np.int32), mask=rng.random(TILE + 1) < 0.1)
    ranks = sess.rank(v, tiebreaker="min", keep_on_device=True)
    idx = sess.call_function("sort_indices", [v], "order=ascending;null_placement=at_end", keep_on_device=True)
    got = sess.call_function("take", [ranks, idx]).to_pylist()
    assert got == sorted(got) and got[0] == 1
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert sorted(got) == sorted(pc.rank(v, sort_keys="ascending", null_placement="at_end", tiebreaker="min").to_pylist())
    # … and a window result's column, taken out of the record batch on the device
    batch = pa.RecordBatch.from_arrays([v], names=["v"])
    dev = sess.window(batch, [], [("v", "asc", "at_end")], ["dense_rank"], keep_on_device=True)
    out = dev.to_arrow()
    assert out.column(0).to_pylist() == pc.rank(v, sort_keys="ascending", tiebreaker="dense").to_pylist()


# ---- rank -------------------------------------------------------------------------------------------------------------------------------
def arrow_rank(arr, order, placement, tiebreaker):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (pyarrow 25 wants the placement inside the sort key; both spellings rank alike)
        return pc.rank(arr, sort_keys=order, null_placement=placement, tiebreaker=tiebreaker)


@pytest.mark.parametrize("tiebreaker", ["min", "first", "dense"])
@pytest.mark.parametrize("order,placement", [("ascending", "at_end"), ("descending", "at_start"), ("ascending", "at_start"), ("descending", "at_end")])
def test_rank_of_arrays_is_arrows(sess, order, placement, tiebreaker):
    rng = np.random.default_rng(12)
    n = TILE + 1
    arrays = [
        pa.array(np.array([np.nan, -0.0, 0.0, 1.0, -2.0, 3.5])[rng.integers(0, 6, n)], mask=rng.random(n) < 0.15),
        pa.array(rng.integers(-20, 20, n).astype(np.int16), mask=rng.random(n) < 0.15),
        pa.array(np.array(["", "a", "ab", "abc", "b"])[rng.integers(0, 5, n)], mask=rng.random(n) < 0.15),
        pa.array(rng.integers(0, 9, 3 * S + 17).astype(np.uint64)),
    ]
    for a in arrays:
        got = sess.rank(a, order=order, null_placement=placement, tiebreaker=tiebreaker)
        assert got.type == pa.uint64() and got.null_count == 0
        assert got.equals(arrow_rank(a, order, placement, tiebreaker)), (a.type, order, placement, tiebreaker)


def test_rank_of_a_record_batch_and_a_chunked_array(sess):
    batch = make_batch(TILE + 1, seed=3)
    names = batch.schema.names
    keys = [(names.index("t"), "asc", "at_end"), (names.index("i"), "desc", "at_end")]
    want = WM.window(batch, [], ORDERS["string_asc_int64_desc"], ["rank", "row_number", "dense_rank"])
    for tb, fn in (("min", "rank"), ("first", "row_number"), ("dense", "dense_rank")):
        assert sess.rank(batch, sort_keys=keys, tiebreaker=tb).to_numpy().tobytes() == want[fn][0].tobytes(), tb
    v = batch.column(names.index("v"))
    chunked = pa.chunked_array([v.slice(0, 1000), v.slice(1000)])
    assert sess.rank(chunked).equals(arrow_rank(v, "ascending", "at_end", "min"))
    assert sess.rank(pa.array([], pa.int32())).to_pylist() == []


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(sess):
    from arrow_go_amd import compute as ac
    batch = make_batch(50, seed=6)

    def refused(err, text, *args, **kw):
        with pytest.raises(err, match=text):
            sess.window(batch, *args, **kw)

    refused(ac.ErrInvalid, "two output columns named 'rank'", [], [], ["rank", "rank"])
    refused(ac.ErrInvalid, "two output columns named 'v_cumulative_sum'", [], [], [("v", "cumulative_sum"), "row_number", ("v", "cumulative_sum")])
    refused(ac.ErrKey, "unknown partition column 'nope'", ["nope"], [], ["rank"])
    refused(ac.ErrKey, "unknown order column 'nope'", [], [("nope", "asc")], ["rank"])
    refused(ac.ErrKey, "unknown column 'nope' of function 'cumulative_max'", [], [], [("nope", "cumulative_max")])
    refused(ac.ErrNotImplemented, "cumulative_sum of column 's'", [], [], [("s", "cumulative_sum")])
    refused(ac.ErrNotImplemented, "cumulative_min of column 'b'", [], [], [("b", "cumulative_min")])
    refused(ac.ErrInvalid, r"more than 7 order keys \(8\)", [], [("k", "asc")] * 8, ["rank"])
    # what the wrapper would not write goes through call_function
    for options, err, text in (("functions=lag:v", ac.ErrInvalid, "unknown function 'lag'"),
                               ("partition_by=g;functions=", ac.ErrInvalid, "no functions"),
                               ("partition_by=g", ac.ErrInvalid, "no functions"),
                               ("", ac.ErrInvalid, "no functions"),
                               ("functions=rank:v", ac.ErrInvalid, "rank takes no column, got 'v'"),
                               ("functions=cumulative_sum", ac.ErrInvalid, "cumulative_sum needs a column")):
        with pytest.raises(err, match=text):
            sess.call_function("window", [batch], options)
    with pytest.raises(ac.ErrInvalid, match="must be a record batch"):
        sess.call_function("window", [batch.column(0)], "functions=rank")
    table = pa.table({"g": pa.chunked_array([[1, 2], [3]])})
    with pytest.raises(ac.ErrInvalid, match=r"column 'g' is chunked \(2 chunks\)"):
        sess.window(table, ["g"], [], ["rank"])
    with pytest.raises(ac.ErrNotImplemented, match="tiebreaker=max"):
        sess.rank(batch.column(0), tiebreaker="max")
    with pytest.raises(ac.ErrInvalid, match="unknown tiebreaker 'average'"):
        sess.call_function("rank", [batch.column(0)], "tiebreaker=average")
    # seven order keys are taken
    assert sess.window(batch, ["g"], [("k", "asc")] * 7, ["rank"]).num_rows == 50


def test_more_than_2_30_rows_are_refused(sess):
    """a Boolean column without a validity buffer: 128 MiB of bits, nothing runs"""
    from arrow_go_amd import compute as ac
    n = (1 << 30) + 1
    col = pa.Array.from_buffers(pa.bool_(), n, [None, pa.py_buffer(np.zeros(n // 8 + 1, np.uint8))], null_count=0)
    batch = pa.RecordBatch.from_arrays([col], names=["b"])
    with pytest.raises(ac.ErrInvalid, match=r"1073741825 rows, more than 2\^30"):
        sess.window(batch, [], [], ["row_number"])
