"""group_by through CallFunction (arrow_go_amd/host/kernels.cc GroupByImpl, Session.group_by), DESIGN.md §3.2.

The yardstick is pyarrow: Table.group_by(keys, use_threads=False).aggregate(aggregates), which returns one row per group, the key
columns first, the aggregates named "<column>_<function>" and "count_all".  Its rows come in first-seen order for small inputs only
(pyarrow 25's grouper inserts the new keys of a mini-batch in an order of its own: with 3000 rows and 41 keys a key first seen in row
24 comes out 37th), so the yardstick's ROWS are put into first-seen order here — the order of first occurrence of the key tuples,
worked out from the input in Python — before the comparison; group_by's own rows are compared as they come.  Whole tables are compared
for EQUALITY, schema included, and NO TOLERANCE is needed: every float value is a multiple of 2^-10 below 2^10 in magnitude, so every group sum of these few
thousand rows is exact in double (and every Float32 value is exact in its 24 bits) — the reproducible fixed-point sum and pyarrow's
sequential sum are then the same number, and so are the two means, one IEEE division of the same operands."""
import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

ALL_SIX = ["sum", "mean", "min", "max", "count"]


@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.close()


def masked(values, rng, p_null, type_=None):
    mask = rng.random(len(values)) < p_null
    return pa.array(values, type=type_, mask=mask) if isinstance(values, np.ndarray) else pa.array([None if m else v for v, m in zip(values, mask)], type=type_)


def first_seen(batch, keys, table):
    """the rows of `table` (one per distinct key tuple of `batch`) in the order in which the tuples first occur in `batch`"""
    order = {}
    for t in zip(*[batch[k].to_pylist() for k in keys]):
        order.setdefault(t, len(order))
    rows = [order[t] for t in zip(*[table[k].to_pylist() for k in keys])]
    assert sorted(rows) == list(range(len(order))), "the groups are not the distinct key tuples"
    return table.take(pa.array(np.argsort(rows), pa.int64())) if rows else table


def check(sess, batch, keys, aggregates):
    keys = [keys] if isinstance(keys, str) else keys
    got = pa.Table.from_batches([sess.group_by(batch, keys, aggregates)])
    want = first_seen(batch, keys, pa.Table.from_batches([batch]).group_by(keys, use_threads=False).aggregate(aggregates).combine_chunks())
    assert got.column_names == want.column_names
    assert got.schema.equals(want.schema), (got.schema, want.schema)
    for name in got.column_names:
        g, w = got[name].combine_chunks(), want[name].combine_chunks()
        assert g.equals(w), (name, g.to_pylist()[:8], w.to_pylist()[:8])
    assert got.equals(want)
    return got


def key_column(kind, n, rng, distinct=40):
    pick = rng.integers(0, distinct, n)
    if kind == "int32":
        return masked((pick * 1000003 - 7).astype(np.int32), rng, 0.05)
    if kind == "string":   # nulls and "" are two keys
        pool = [""] + ["k%d" % (i * i) for i in range(1, distinct)]
        return masked([pool[i] for i in pick], rng, 0.05, pa.string())
    if kind == "large_binary":
        pool = [b"", b"\0", b"\0\0"] + [bytes([i, 255 - i]) * (i % 5 + 1) for i in range(3, distinct)]
        return masked([pool[i] for i in pick], rng, 0.05, pa.large_binary())
    if kind == "fixed3":
        return masked([bytes([i, i // 2, 7]) for i in pick], rng, 0.05, pa.binary(3))
    if kind == "decimal128":
        import decimal
        return masked([decimal.Decimal(int(i) * 10**20 - 5).scaleb(-3) for i in pick], rng, 0.05, pa.decimal128(30, 3))
    if kind == "bool":
        return masked([bool(i & 1) for i in pick], rng, 0.2, pa.bool_())
    if kind == "timestamp":
        return masked((pick.astype(np.int64) * 86_400_000_000 + 1_600_000_000_000_000), rng, 0.05).cast(pa.timestamp("us", tz="UTC"))
    if kind == "int16":
        return masked((pick - 20).astype(np.int16), rng, 0.05)
    if kind == "int64":
        return masked(pick.astype(np.int64) << 40, rng, 0.05)
    raise AssertionError(kind)


def value_column(dtype, n, rng, p_null=0.15):
    if np.dtype(dtype).kind == "f":
        return masked((rng.integers(-2**19, 2**19, n) / 1024).astype(dtype), rng, p_null)
    info = np.iinfo(dtype)
    return masked(rng.integers(max(info.min, -2**40), min(info.max, 2**40), n).astype(dtype), rng, p_null)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["int32", "string", "large_binary", "fixed3", "decimal128", "bool", "timestamp"])
def test_one_key_of_every_kind(sess, kind):
    rng = np.random.default_rng(3)
    n = 3000
    batch = pa.record_batch({"k": key_column(kind, n, rng), "v": value_column(np.int32, n, rng), "w": value_column(np.float64, n, rng)})
    got = check(sess, batch, ["k"], [("v", "sum"), ("w", "mean"), ("v", "count"), ([], "count_all")])
    assert got["k"].type == batch["k"].type and got["k"].null_count == 1


@pytest.mark.gpu
def test_two_keys_with_nulls_in_both_and_tuples_that_do_and_do_not_pack(sess):
    rng = np.random.default_rng(5)
    n = 4000
    batch = pa.record_batch({"s": key_column("string", n, rng, 9), "h": key_column("int16", n, rng, 7), "i": key_column("int32", n, rng, 5),
                             "l": key_column("int64", n, rng, 6), "v": value_column(np.int8, n, rng)})
    aggs = [("v", "sum"), ("v", "min"), ([], "count_all")]
    check(sess, batch, ["s", "h"], aggs)            # (String, Int16): compared column by column
    check(sess, batch, ["i", "h"], aggs)            # 32 + 16 value bits + 2 validity bits: one packed 8-byte word
    check(sess, batch, ["l", "i"], aggs)            # 96 bits: does not pack
    check(sess, batch, ["h", "s", "i", "l"], aggs)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int8, np.uint16, np.int32, np.uint64, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_all_six_aggregates(sess, dtype):
    rng = np.random.default_rng(7)
    n = 5000
    keys = key_column("int32", n, rng, 100)
    # the group of the first row has no valid value: sum, mean, min and max are null there, count is 0
    first = keys[0].as_py()
    hit = np.array([k == first for k in keys.to_pylist()])
    plain = value_column(dtype, n, rng, p_null=0)
    vals = pa.array(plain.to_numpy(), mask=hit | (rng.random(n) < 0.15))
    batch = pa.record_batch({"k": keys, "v": vals})
    got = check(sess, batch, ["k"], [("v", a) for a in ALL_SIX] + [([], "count_all")])
    row = got.slice(0, 1).to_pylist()[0]
    assert [row["v_" + a] for a in ALL_SIX] == [None, None, None, None, 0] and row["count_all"] == int(hit.sum())
    # a sliced batch: every column at an offset, the validity bitmaps at a bit offset
    check(sess, batch.slice(13), ["k"], [("v", a) for a in ALL_SIX])


@pytest.mark.gpu
def test_edge_shapes(sess):
    rng = np.random.default_rng(9)
    n = 3000
    aggs = [("v", a) for a in ALL_SIX] + [([], "count_all")]
    v = value_column(np.float32, n, rng)
    s = pa.array(["x"] * n)
    own = pa.array(rng.permutation(n).astype(np.int32))
    batch = pa.record_batch({"one": s, "own": own, "v": v})
    assert check(sess, batch, ["one"], aggs).num_rows == 1            # every row in one group
    assert check(sess, batch, ["own"], aggs).num_rows == n            # every row its own group
    assert check(sess, batch.slice(0, 1), ["own", "one"], aggs).num_rows == 1
    empty = check(sess, batch.slice(0, 0), ["one", "own"], aggs)      # no rows: the schema, no groups
    assert empty.num_rows == 0 and empty.schema.names == ["one", "own"] + ["v_" + a for a in ALL_SIX] + ["count_all"]
    assert check(sess, batch, ["own"], []).num_rows == n              # no aggregates: the distinct keys


@pytest.mark.gpu
def test_min_max_of_a_timestamp_keeps_the_type_and_count_takes_any_column(sess):
    rng = np.random.default_rng(11)
    n = 2000
    batch = pa.record_batch({"k": key_column("bool", n, rng), "t": key_column("timestamp", n, rng), "d": masked(rng.integers(0, 20000, n).astype(np.int32), rng, 0.3).cast(pa.date32()),
                             "s": key_column("string", n, rng), "b": key_column("bool", n, rng), "x": key_column("decimal128", n, rng)})
    got = check(sess, batch, ["k"], [("t", "min"), ("t", "max"), ("d", "min"), ("d", "max"), ("t", "count"), ("s", "count"), ("b", "count"), ("x", "count")])
    assert got["t_min"].type == pa.timestamp("us", tz="UTC") and got["d_max"].type == pa.date32()


@pytest.mark.gpu
def test_refusals(sess):
    from arrow_go_amd import compute as ac
    rng = np.random.default_rng(13)
    n = 100
    batch = pa.record_batch({"k": key_column("int32", n, rng), "s": key_column("string", n, rng), "v": value_column(np.int32, n, rng),
                             "t": key_column("timestamp", n, rng), "d": key_column("string", n, rng).dictionary_encode()})
    for agg in ("sum", "mean", "min", "max"):
        with pytest.raises(ac.ErrNotImplemented, match="no kernel matching input types"):
            sess.group_by(batch, ["k"], [("s", agg)])
    with pytest.raises(ac.ErrNotImplemented, match="no kernel matching input types"):
        sess.group_by(batch, ["k"], [("t", "sum")])
    with pytest.raises(ac.ErrNotImplemented, match="dictionary-typed key column 'd'"):
        sess.group_by(batch, ["k", "d"], [("v", "sum")])
    with pytest.raises(ac.ErrInvalid, match="unknown key column 'nope'"):
        sess.group_by(batch, ["k", "nope"], [("v", "sum")])
    with pytest.raises(ac.ErrInvalid, match="unknown column 'gone'"):
        sess.group_by(batch, ["k"], [("gone", "sum")])
    with pytest.raises(ac.ErrInvalid, match="unknown aggregate 'median'"):
        sess.group_by(batch, ["k"], [("v", "median")])
    with pytest.raises(ac.ErrInvalid, match="no keys"):
        sess.call_function("group_by", [batch], "keys=;aggregates=sum:v")
    with pytest.raises(ac.ErrInvalid, match="no keys"):
        sess.call_function("group_by", [batch], "")
    with pytest.raises(ac.ErrInvalid, match="more than 8 keys"):
        sess.group_by(batch, ["k"] * 9, [("v", "sum")])
    with pytest.raises(ac.ErrInvalid, match="record batch"):
        sess.call_function("group_by", [batch["k"]], "keys=k")


@pytest.mark.gpu
def test_the_wrapper_writes_the_option_string(sess):
    rng = np.random.default_rng(15)
    n = 500
    batch = pa.record_batch({"a": key_column("string", n, rng), "b": key_column("int16", n, rng), "v": value_column(np.uint16, n, rng)})
    by_hand = sess.call_function("group_by", [batch], "keys=a,b;aggregates=sum:v,mean:v,min:v,max:v,count:v,count_all")
    wrapped = sess.group_by(batch, ["a", "b"], [("v", a) for a in ALL_SIX] + [([], "count_all")])
    assert wrapped.equals(by_hand) and wrapped.schema.equals(by_hand.schema)
    assert sess.group_by(batch, "a", [("v", "count")]).equals(sess.call_function("group_by", [batch], "keys=a;aggregates=count:v"))
