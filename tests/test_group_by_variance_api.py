"""variance, stddev and count_distinct of group_by through CallFunction (host/kernels.cc GroupByImpl, Session.group_by), DESIGN.md §3.2.

The yardstick is pyarrow's Table.group_by(keys).aggregate(...), whole tables compared for EQUALITY, schema included, its rows put into
first-seen order as tests/test_group_by_api.py does it.  No tolerance: the inputs are group_variance_model.exact_inputs — valid counts
that are powers of two, values that are multiples of 16 — on which every intermediate of the variance is exact, so that pyarrow's
result is the exact rational variance rounded once (tests/test_group_variance_model_host.py), which is the definition's."""
import decimal

import numpy as np
import pytest

from tests import group_variance_model as M

pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc   # noqa: E402

MOMENTS = ("variance", "stddev")


@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.close()


def first_seen(batch, keys, table):
    """the rows of `table` (one per distinct key tuple of `batch`) in the order in which the tuples first occur in `batch`"""
    order = {}
    for t in zip(*[batch[k].to_pylist() for k in keys]):
        order.setdefault(t, len(order))
    rows = [order[t] for t in zip(*[table[k].to_pylist() for k in keys])]
    assert sorted(rows) == list(range(len(order))), "the groups are not the distinct key tuples"
    return table.take(pa.array(np.argsort(rows), pa.int64())) if rows else table


def check(sess, batch, keys, aggregates):
    """aggregates as Session.group_by takes them; pyarrow gets the ddof as VarianceOptions"""
    want_aggs = [(a[0], a[1], pc.VarianceOptions(ddof=a[2] if len(a) == 3 else 0)) if a[1] in MOMENTS else a for a in aggregates]
    got = pa.Table.from_batches([sess.group_by(batch, keys, aggregates)])
    want = first_seen(batch, keys, pa.Table.from_batches([batch]).group_by(keys, use_threads=False).aggregate(want_aggs).combine_chunks())
    assert got.column_names == want.column_names
    assert got.schema.equals(want.schema), (got.schema, want.schema)
    for i, name in enumerate(got.column_names):
        g, w = got.column(i).combine_chunks(), want.column(i).combine_chunks()
        assert g.equals(w), (name, g.to_pylist()[:8], w.to_pylist()[:8])
    assert got.equals(want)
    return got


def exact_batch(dtype, key_kind, seed, lead=0):
    """-> (record batch with the key column(s) and "v", key names): 200 groups, the group of the first row without a valid value;
    `lead` rows of other groups in front, for a caller that slices them away"""
    rng = np.random.default_rng(seed)
    ids, vals, valid = M.exact_inputs(dtype, rng, 200)
    valid[ids == ids[0]] = False
    if lead:
        ids = np.concatenate([rng.integers(500, 520, lead).astype(np.int32), ids])
        vals = np.concatenate([np.full(lead, 48, vals.dtype), vals])
        valid = np.concatenate([rng.random(lead) < 0.5, valid])
    v = pa.array(vals, mask=~valid)
    if key_kind == "int32":
        return pa.record_batch({"k": pa.array((ids * 1000003 - 7).astype(np.int32)), "v": v}), ["k"]
    if key_kind == "string":
        return pa.record_batch({"k": pa.array(["" if i == 3 else "k%d" % (i * i) for i in ids], pa.string()), "v": v}), ["k"]
    assert key_kind == "tuple"
    return pa.record_batch({"a": pa.array((ids % 7).astype(np.int16)), "b": pa.array(["g%d" % (i // 7) for i in ids], pa.string()), "v": v}), ["a", "b"]


def moment_aggs(ddof):
    return [("v", "variance", ddof), ("v", "stddev", ddof), ("v", "sum"), ("v", "mean"), ("v", "count")]


@pytest.mark.gpu
@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("dtype,key_kind", [(np.int8, "int32"), (np.uint16, "string"), (np.int32, "tuple"), (np.int64, "int32"), (np.float32, "string"),
                                            (np.float64, "tuple")], ids=lambda p: p if isinstance(p, str) else np.dtype(p).name)
def test_variance_and_stddev_equal_pyarrow(sess, dtype, key_kind, ddof):
    batch, keys = exact_batch(dtype, key_kind, seed=3)
    got = check(sess, batch, keys, moment_aggs(ddof))
    row = got.slice(0, 1).to_pylist()[0]      # the group of the first row has no valid value
    assert [row["v_variance"], row["v_stddev"], row["v_sum"], row["v_mean"], row["v_count"]] == [None, None, None, None, 0]
    assert got["v_variance"].type == pa.float64() and got["v_stddev"].type == pa.float64()
    if ddof == 1:                             # a single valid value: null at ddof 1, and only there beside the empty group
        assert got["v_variance"].null_count == sum(c <= 1 for c in got["v_count"].to_pylist()) > 1


@pytest.mark.gpu
def test_variance_alone_two_ddofs_and_a_column_without_nulls(sess):
    batch, keys = exact_batch(np.int32, "int32", seed=5)
    check(sess, batch, keys, [("v", "variance")])
    check(sess, batch, keys, [("v", "stddev", 1), ("v", "variance", 0), ("v", "variance", 1), ("v", "count")])
    dense = batch.filter(batch["v"].is_valid())               # (the valid counts stay powers of two)
    dense = pa.record_batch({"k": dense["k"], "v": pa.array(dense["v"].to_numpy())})
    assert dense["v"].null_count == 0 and dense["v"].buffers()[0] is None
    check(sess, dense, keys, [("v", "variance", 1), ("v", "stddev")])   # ddof 1 without a validity bitmap: nulls from the counts alone


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int8, np.float64], ids=lambda d: np.dtype(d).name)
def test_a_sliced_batch_and_no_rows(sess, dtype):
    batch, keys = exact_batch(dtype, "tuple", seed=7, lead=13)
    check(sess, batch.slice(13), keys, moment_aggs(1))      # every column at an offset, the validity bitmap at a bit offset
    empty = check(sess, batch.slice(0, 0), keys, moment_aggs(0) + [("v", "count_distinct")])
    assert empty.num_rows == 0 and empty.schema.names == keys + ["v_variance", "v_stddev", "v_sum", "v_mean", "v_count", "v_count_distinct"]


def masked(values, rng, p_null, type_):
    return pa.array([None if m else v for v, m in zip(values, rng.random(len(values)) < p_null)], type=type_)


@pytest.mark.gpu
def test_count_distinct_equals_pyarrow(sess):
    rng = np.random.default_rng(9)
    n = 3000
    pick = lambda k: rng.integers(0, k, n)   # noqa: E731
    batch = pa.record_batch({
        "k": masked((pick(40) * 1000003 - 7).tolist(), rng, 0.05, pa.int32()),
        "i": masked((pick(9) * 77 - 300).tolist(), rng, 0.2, pa.int32()),
        "s": masked([["", "a", "ab", "b", "a\0"][j] for j in pick(5)], rng, 0.2, pa.string()),
        "b": masked([bool(j) for j in pick(2)], rng, 0.3, pa.bool_()),
        "f": masked([bytes([j, j // 2, 7]) for j in pick(6)], rng, 0.2, pa.binary(3)),
        "d": masked([decimal.Decimal(int(j) * 10**20 - 5).scaleb(-3) for j in pick(7)], rng, 0.2, pa.decimal128(30, 3)),
        "allnull": pa.array([None] * n, pa.int32()),
    })
    aggs = [(c, "count_distinct") for c in ("i", "s", "b", "f", "d", "allnull")]
    got = check(sess, batch, ["k"], aggs + [("i", "count"), ("i", "min")])
    assert got["i_count_distinct"].type == pa.int64() and all(got[c + "_count_distinct"].null_count == 0 for c, _ in aggs)
    assert not any(got["allnull_count_distinct"].to_pylist())
    check(sess, batch.slice(29), ["k"], aggs)
    check(sess, batch, ["k", "b"], [("s", "count_distinct"), ("k", "count_distinct")])


@pytest.mark.gpu
def test_count_distinct_compares_bytes(sess):
    batch = pa.record_batch({"k": pa.array([1, 1, 1, 2, 2], pa.int32()), "v": pa.array([0.0, -0.0, 0.0, -0.0, None], pa.float64())})
    got = sess.group_by(batch, ["k"], [("v", "count_distinct")])
    assert got["v_count_distinct"].to_pylist() == [2, 1]      # −0.0 and +0.0 are two values


@pytest.mark.gpu
def test_the_option_string_carries_ddof_as_a_third_field(sess):
    batch, keys = exact_batch(np.float32, "int32", seed=11)
    wrapped = sess.group_by(batch, keys, [("v", "variance", 1), ("v", "stddev", 1), ("v", "variance"), ("v", "count_distinct")])
    by_hand = sess.call_function("group_by", [batch], "keys=k;aggregates=variance:v:1,stddev:v:1,variance:v,count_distinct:v")
    assert wrapped.equals(by_hand) and wrapped.schema.equals(by_hand.schema)
    assert sess.call_function("group_by", [batch], "keys=k;aggregates=variance:v:0").equals(sess.group_by(batch, keys, [("v", "variance")]))
    assert not wrapped.column(1).equals(wrapped.column(3))


@pytest.mark.gpu
def test_refusals(sess):
    from arrow_go_amd import compute as ac
    n = 50
    batch = pa.record_batch({"k": pa.array(np.arange(n, dtype=np.int32) % 5), "v": pa.array(np.arange(n, dtype=np.int32)),
                             "s": pa.array(["x%d" % (i % 3) for i in range(n)]),
                             "t": pa.array(np.arange(n, dtype=np.int64)).cast(pa.timestamp("us", tz="UTC")),
                             "x": pa.array([decimal.Decimal(i) for i in range(n)], pa.decimal128(20, 2)),
                             "d": pa.array(["x%d" % (i % 3) for i in range(n)]).dictionary_encode()})
    for col in ("s", "t", "x"):
        for fn in MOMENTS:
            with pytest.raises(ac.ErrNotImplemented, match="no kernel matching input types"):
                sess.group_by(batch, ["k"], [(col, fn)])
    with pytest.raises(ac.ErrNotImplemented, match="dictionary-typed column 'd'"):
        sess.group_by(batch, ["k"], [("d", "count_distinct")])
    for text in ("variance:v:-1", "variance:v:x", "stddev:v:", "variance:v:1:2", "sum:v:1", "count_distinct:v:0"):
        with pytest.raises(ac.ErrInvalid, match="ddof"):
            sess.call_function("group_by", [batch], "keys=k;aggregates=" + text)
    for agg in (("v", "sum", 1), ("v", "variance", -1), ("v", "variance", 1.5), ("v", "variance", 1, 2)):
        with pytest.raises(ValueError):
            sess.group_by(batch, ["k"], [agg])
