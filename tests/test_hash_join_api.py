"""hash_join through CallFunction (arrow_go_amd/host/kernels.cc HashJoinImpl, Session.hash_join), DESIGN.md §3.2a.

Two yardsticks.
1. THE CONTRACT, a dict-based model in Python: a dict from the right side's key tuples to their row lists, then a loop over the left
   rows in order.  It returns the exact table hash_join must return — columns, types, and the documented row order (left rows
   ascending, the right matches of one left row ascending, an unmatched left row of a left outer join in its place with nulls on the
   right) — and the comparison is Table.equals, schema included.  Keys are compared as hash_join compares them: by their bytes, so a
   float key takes part as its bit pattern (-0.0 and +0.0 differ, NaNs with equal payloads are equal); a null never matches.
2. pyarrow's Table.join(..., use_threads=False).  Its row order is unspecified, so both tables are compared after their rows have
   been sorted by all columns.  Every case takes this comparison as well, except the cases with ±0.0 or NaN in a float key, where
   pyarrow's key equality is another one; those are listed in PYARROW_LEFT_OUT, and a test counts them.

Payloads are integers, strings and Booleans: no tolerance anywhere.  Both sides of every case are slices that start at row 3, so
every buffer offset and every bitmap bit offset is non-zero."""
import ctypes as C
import decimal

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")

JOIN_TYPES = ["inner", "left_outer", "left_semi", "left_anti"]
PYARROW_NAME = {"inner": "inner", "left_outer": "left outer", "left_semi": "left semi", "left_anti": "left anti"}
KEY_KINDS = ["int32", "int64", "string", "large_binary", "fixed3", "decimal128", "bool", "timestamp"]
PYARROW_LEFT_OUT = {"float64_zeros_and_nans", "float32_zeros_and_nans"}   # ±0.0 / NaN in a float key: the model only
compared_with_pyarrow, left_to_the_model = set(), set()


@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.close()


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def masked(values, rng, p_null, type_=None):
    mask = rng.random(len(values)) < p_null
    return pa.array(values, type=type_, mask=mask) if isinstance(values, np.ndarray) else pa.array([None if m else v for v, m in zip(values, mask)], type=type_)


def key_column(kind, pick, rng, p_null=0.05):
    """key number pick[i] as a value of the kind, nulls sprinkled in: equal numbers are equal keys on both sides"""
    if kind == "int32":
        return masked((pick * 1000003 - 7).astype(np.int32), rng, p_null)
    if kind == "int64":
        return masked(pick.astype(np.int64) << 40, rng, p_null)
    if kind == "int16":
        return masked((pick - 20).astype(np.int16), rng, p_null)
    if kind == "string":   # "" is a key like any other
        return masked(["" if i == 0 else "k%d" % (i * i) for i in pick], rng, p_null, pa.string())
    if kind == "large_binary":
        return masked([b"" if i == 0 else bytes([i % 256, 255 - i % 256]) * (i % 5 + 1) for i in pick], rng, p_null, pa.large_binary())
    if kind == "fixed3":
        return masked([bytes([i % 256, i // 2 % 256, 7]) for i in pick], rng, p_null, pa.binary(3))
    if kind == "decimal128":
        return masked([decimal.Decimal(int(i) * 10**20 - 5).scaleb(-3) for i in pick], rng, p_null, pa.decimal128(30, 3))
    if kind == "bool":
        return masked([bool(i & 1) for i in pick], rng, p_null, pa.bool_())
    if kind == "timestamp":
        return masked((pick.astype(np.int64) * 86_400_000_000 + 1_600_000_000_000_000), rng, p_null).cast(pa.timestamp("us", tz="UTC"))
    raise AssertionError(kind)


def sliced(columns):
    """the record batch of the columns as a slice that starts at row 3 of a longer one"""
    longer = {}
    for name, col in columns.items():
        junk = col.slice(0, min(5, len(col)))
        if len(junk) < 5:
            junk = pa.concat_arrays([junk] + [pa.nulls(5 - len(junk), col.type)])
        longer[name] = pa.concat_arrays([junk.slice(0, 3), col, junk.slice(3, 2)])
    n = len(next(iter(columns.values())))
    batch = pa.record_batch(longer).slice(3, n)
    assert batch.num_rows == n and all(c.offset == 3 for c in batch.columns)
    return batch


def two_sides(kinds, n_left, n_right, seed, left_names=("k",), right_names=None, distinct=60, p_null=0.05):
    """key numbers 0 .. distinct + 19 on the left, 20 .. distinct + 39 on the right: some keys on one side only, duplicates on both"""
    rng = np.random.default_rng(seed)
    right_names = right_names or left_names
    lpick = [rng.integers(0, distinct + 20, n_left) for _ in kinds]
    rpick = [rng.integers(20, distinct + 40, n_right) for _ in kinds]
    left = {name: key_column(kind, p, rng, p_null) for name, kind, p in zip(left_names, kinds, lpick)}
    right = {name: key_column(kind, p, rng, p_null) for name, kind, p in zip(right_names, kinds, rpick)}
    left["lv"] = pa.array(np.arange(n_left, dtype=np.int64))
    left["ls"] = masked(["L%d" % (i % 97) for i in range(n_left)], rng, 0.1, pa.string())
    right["rv"] = masked(rng.integers(-1000, 1000, n_right).astype(np.int32), rng, 0.1)
    right["rs"] = masked(["" if i % 11 == 0 else "R%d" % (i % 89) * (i % 4) for i in range(n_right)], rng, 0.1, pa.string())
    right["rb"] = masked([bool((i * 7) & 2) for i in range(n_right)], rng, 0.1, pa.bool_())
    return sliced(left), sliced(right)


# ---- yardstick 1: the contract ------------------------------------------------------------------------------------------------------
def key_tuples(batch, names):
    """one tuple per row, None in it where a key is null; float keys by their bit pattern"""
    cols = []
    for name in names:
        col = batch[name]
        if pa.types.is_floating(col.type):
            bits = np.frombuffer(col.buffers()[1], np.uint32 if col.type == pa.float32() else np.uint64, len(col), col.offset * col.type.bit_width // 8)
            cols.append([int(b) if v else None for b, v in zip(bits, col.is_valid().to_pylist())])
        else:
            cols.append(col.to_pylist())
    return list(zip(*cols))


def model_join(left, right, left_keys, right_keys, join_type):
    build = {}
    for j, t in enumerate(key_tuples(right, right_keys)):
        if None not in t:
            build.setdefault(t, []).append(j)
    lrows, rrows = [], []
    for i, t in enumerate(key_tuples(left, left_keys)):
        matches = build.get(t, []) if None not in t else []
        if join_type == "left_semi":
            lrows += [i] if matches else []
        elif join_type == "left_anti":
            lrows += [] if matches else [i]
        else:
            if not matches and join_type == "left_outer":
                matches = [None]
            lrows += [i] * len(matches)
            rrows += matches
    lt = pa.Table.from_batches([left]).take(pa.array(lrows, pa.int64()))
    if join_type in ("left_semi", "left_anti"):
        return lt.combine_chunks()
    rt = pa.Table.from_batches([right]).drop_columns(list(right_keys)).take(pa.array(rrows, pa.int64()))
    for name in rt.column_names:
        lt = lt.append_column(rt.schema.field(name), rt[name])
    return lt.combine_chunks()


# ---- yardstick 2: pyarrow ------------------------------------------------------------------------------------------------------------
def sorted_rows(table, names):
    def key(row):
        return tuple((v is None, 0 if v is None else v) for v in row)
    return sorted(zip(*[table[n].to_pylist() for n in names]), key=key)


def pyarrow_join(left, right, left_keys, right_keys, join_type):
    return pa.Table.from_batches([left]).join(pa.Table.from_batches([right]), keys=list(left_keys), right_keys=list(right_keys),
                                              join_type=PYARROW_NAME[join_type], use_threads=False)


def same_column(g, w):
    """Array.equals — for a float column with the NaNs compared too: equal validity, and equal BITS under the valid slots"""
    if not pa.types.is_floating(g.type):
        return g.equals(w)
    if g.type != w.type or len(g) != len(w) or g.is_valid().to_pylist() != w.is_valid().to_pylist():
        return False
    u = np.uint32 if g.type == pa.float32() else np.uint64
    keep = np.array(g.is_valid().to_pylist(), bool)
    bits = [np.frombuffer(a.buffers()[1], u, len(a), a.offset * np.dtype(u).itemsize)[keep] for a in (g, w)]
    return bool((bits[0] == bits[1]).all())


def check(sess, case, left, right, left_keys, right_keys=None, join_types=JOIN_TYPES):
    left_keys = [left_keys] if isinstance(left_keys, str) else list(left_keys)
    rkeys = left_keys if right_keys is None else ([right_keys] if isinstance(right_keys, str) else list(right_keys))
    out = {}
    for jt in join_types:
        got = pa.Table.from_batches([sess.hash_join(left, right, left_keys, right_keys, jt)])
        want = model_join(left, right, left_keys, rkeys, jt)
        assert got.column_names == want.column_names, (jt, got.column_names)
        assert got.schema.equals(want.schema), (jt, got.schema, want.schema)
        for name in got.column_names:
            g, w = got[name].combine_chunks(), want[name].combine_chunks()
            assert same_column(g, w), (jt, name, got.num_rows, want.num_rows, g.to_pylist()[:8], w.to_pylist()[:8])
        plain = [n for n in got.column_names if not pa.types.is_floating(got.schema.field(n).type)]
        assert got.select(plain).equals(want.select(plain)), jt
        if case in PYARROW_LEFT_OUT:
            left_to_the_model.add(case)
        else:
            other = pyarrow_join(left, right, left_keys, rkeys, jt)
            assert sorted(other.column_names) == sorted(got.column_names), (jt, other.column_names)
            assert sorted_rows(got, got.column_names) == sorted_rows(other, got.column_names), jt
            for name in got.column_names:
                assert other.schema.field(name).type == got.schema.field(name).type, (jt, name)
            compared_with_pyarrow.add(case)
        out[jt] = got
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KEY_KINDS)
def test_one_key_of_every_kind_with_every_join_type(sess, kind):
    left, right = two_sides([kind], 3000, 2500, seed=KEY_KINDS.index(kind), distinct=2 if kind == "bool" else 60)
    if kind == "bool":   # two keys only: keep the product small
        left, right = left.slice(0, 300), right.slice(0, 200)
    out = check(sess, "kind_" + kind, left, right, "k")
    assert out["inner"]["k"].type == left["k"].type
    assert 0 < out["left_semi"].num_rows < left.num_rows and out["left_semi"].num_rows + out["left_anti"].num_rows == left.num_rows
    assert out["left_outer"].num_rows > out["inner"].num_rows > left.num_rows // 2       # runs longer than 1, and unmatched rows
    assert out["left_outer"]["rs"].null_count > 0 and out["left_outer"]["rb"].null_count > 0


@pytest.mark.gpu
def test_two_column_keys_with_nulls_in_either_component(sess):
    left, right = two_sides(["int16", "string"], 4000, 3000, seed=21, left_names=("h", "s"), distinct=8, p_null=0.1)
    out = check(sess, "two_columns", left, right, ["h", "s"])
    lt = key_tuples(left, ["h", "s"])
    assert any(t[0] is None and t[1] is not None for t in lt) and any(t[1] is None and t[0] is not None for t in lt)
    assert 0 < out["inner"].num_rows and out["left_anti"].num_rows > 0


@pytest.mark.gpu
def test_differently_named_keys(sess):
    left, right = two_sides(["int64", "string"], 2000, 2000, seed=22, left_names=("a", "b"), right_names=("x", "y"), distinct=12)
    out = check(sess, "other_names", left, right, ["a", "b"], ["x", "y"])
    assert out["left_outer"].column_names == ["a", "b", "lv", "ls", "rv", "rs", "rb"]
    # one name given as a plain string
    left1, right1 = two_sides(["int32"], 500, 500, seed=23, left_names=("a",), right_names=("x",))
    check(sess, "other_names_single", left1, right1, "a", "x", ["inner", "left_anti"])


@pytest.mark.gpu
def test_empty_sides_and_no_key_in_common(sess):
    left, right = two_sides(["int32"], 1500, 1200, seed=24)
    for jt, rows in check(sess, "empty_left", left.slice(0, 0), right, "k").items():
        assert rows.num_rows == 0
    out = check(sess, "empty_right", left, right.slice(0, 0), "k")
    assert [out[jt].num_rows for jt in JOIN_TYPES] == [0, 1500, 0, 1500] and out["left_outer"]["rv"].null_count == 1500
    check(sess, "both_empty", left.slice(0, 0), right.slice(0, 0), "k")
    rng = np.random.default_rng(25)
    apart_l = sliced({"k": pa.array(rng.integers(0, 100, 1000).astype(np.int32)), "lv": pa.array(np.arange(1000, dtype=np.int64))})
    apart_r = sliced({"k": pa.array(rng.integers(100, 200, 900).astype(np.int32)), "rs": pa.array(["r%d" % i for i in range(900)])})
    out = check(sess, "nothing_in_common", apart_l, apart_r, "k")
    assert [out[jt].num_rows for jt in JOIN_TYPES] == [0, 1000, 0, 1000]


@pytest.mark.gpu
def test_keys_all_null_on_one_side(sess):
    left, right = two_sides(["string"], 800, 700, seed=26)
    nulls = pa.nulls(700, pa.string())
    right_null = sliced({"k": nulls, "rv": right["rv"], "rs": right["rs"], "rb": right["rb"]})
    out = check(sess, "right_keys_all_null", left, right_null, "k")
    assert [out[jt].num_rows for jt in JOIN_TYPES] == [0, 800, 0, 800]
    left_null = sliced({"k": pa.nulls(800, pa.string()), "lv": left["lv"], "ls": left["ls"]})
    out = check(sess, "left_keys_all_null", left_null, right, "k")
    assert [out[jt].num_rows for jt in JOIN_TYPES] == [0, 800, 0, 800]
    # null on both sides: a null does not match a null
    out = check(sess, "both_keys_all_null", left_null, right_null, "k")
    assert out["inner"].num_rows == 0 and out["left_anti"].num_rows == 800


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_float_keys_are_their_bytes(sess, dtype):
    """-0.0 and +0.0 are two keys; NaNs with equal payloads are one key, NaNs with different payloads are not"""
    rng = np.random.default_rng(27)
    u = np.uint64 if dtype == np.float64 else np.uint32
    quiet = np.array([0x7FF8000000000000 if dtype == np.float64 else 0x7FC00000], u).view(dtype)[0]
    other = np.array([0x7FF8000000000001 if dtype == np.float64 else 0x7FC00001], u).view(dtype)[0]
    pool = np.array([0.0, -0.0, quiet, other, 1.5, -2.25, np.inf], dtype)
    lk, rk = pool[rng.integers(0, 7, 600)], pool[np.r_[rng.integers(0, 3, 300), rng.integers(4, 7, 200)]]     # `other` on the left only
    left = sliced({"k": masked(lk, rng, 0.05), "lv": pa.array(np.arange(600, dtype=np.int64))})
    right = sliced({"k": masked(rk, rng, 0.05), "rs": pa.array(["r%d" % i for i in range(500)])})
    name = np.dtype(dtype).name + "_zeros_and_nans"
    out = check(sess, name, left, right, "k")
    anti = out["left_anti"]["k"].combine_chunks()
    bits = set(np.frombuffer(anti.buffers()[1], u, len(anti), anti.offset * np.dtype(u).itemsize)[np.array(anti.is_valid().to_pylist(), bool)].tolist())
    assert bits == {int(np.array([other], dtype).view(u)[0])}       # the only valid left key without a partner
    semi = out["left_semi"]["k"].to_numpy(zero_copy_only=False)
    assert np.isnan(semi).any() and (np.signbit(semi) & (semi == 0)).any() and (~np.signbit(semi) & (semi == 0)).any()


@pytest.mark.gpu
def test_the_wrapper_writes_the_option_string(sess):
    left, right = two_sides(["int32"], 700, 600, seed=28)
    by_hand = sess.call_function("hash_join", [left, right], "left_keys=k")
    wrapped = sess.hash_join(left, right, "k")
    assert wrapped.equals(by_hand) and wrapped.schema.equals(by_hand.schema) and wrapped.num_rows > 0
    assert sess.hash_join(left, right, ["k"], ["k"], "left_outer").equals(sess.call_function("hash_join", [left, right], "left_keys=k;right_keys=k;type=left_outer"))
    assert sess.hash_join(left, right, "k", join_type="left_anti").equals(sess.call_function("hash_join", [left, right], "type=left_anti;left_keys=k"))
    kept = sess.hash_join(left, right, "k", keep_on_device=True)
    assert kept.to_arrow().equals(wrapped)
    kept.release()
    for bad in ("a,b", "a;b", "a=b"):
        with pytest.raises(ValueError, match="options string"):
            sess.hash_join(left, right, bad)
        with pytest.raises(ValueError, match="options string"):
            sess.hash_join(left, right, "k", [bad])


@pytest.mark.gpu
def test_temporal_labels(sess):
    from arrow_go_amd import compute as ac
    left, right = two_sides(["timestamp"], 400, 300, seed=29)
    got = sess.hash_join(left, right, "k", join_type="left_outer")
    assert got.schema.field("k").type == pa.timestamp("us", tz="UTC")
    other = pa.record_batch({"k": right["k"].cast(pa.int64()).cast(pa.timestamp("ms", tz="UTC")), "rv": right["rv"]})
    with pytest.raises(ac.ErrNotImplemented, match="no kernel matching input types"):
        sess.hash_join(left, other, "k")
    plain = pa.record_batch({"k": right["k"].cast(pa.int64()), "rv": right["rv"]})
    with pytest.raises(ac.ErrNotImplemented, match="no kernel matching input types"):
        sess.hash_join(left, plain, "k")


@pytest.mark.gpu
def test_refusals(sess):
    from arrow_go_amd import compute as ac
    left, right = two_sides(["int32"], 100, 80, seed=30)
    invalid = [
        (lambda: sess.call_function("hash_join", [left["k"], right], "left_keys=k"), "record batches"),
        (lambda: sess.call_function("hash_join", [left, right["k"]], "left_keys=k"), "record batches"),
        (lambda: sess.call_function("hash_join", [left, right], ""), "no keys"),
        (lambda: sess.call_function("hash_join", [left, right], "left_keys=;type=inner"), "no keys"),
        (lambda: sess.call_function("hash_join", [left, right], "right_keys=k"), "no keys"),
        (lambda: sess.hash_join(left, right, ["k"] * 9), "more than 8 keys"),
        (lambda: sess.hash_join(left, right, ["k", "lv"], ["k"]), "2 left keys but 1 right keys"),
        (lambda: sess.hash_join(left, right, "nope"), "unknown key column 'nope' of the left batch"),
        (lambda: sess.hash_join(left, right, "k", "gone"), "unknown key column 'gone' of the right batch"),
        (lambda: sess.hash_join(left, right, "k", join_type="right_outer"), "unknown type 'right_outer'"),
        (lambda: sess.hash_join(left, pa.record_batch({"k": right["k"], "lv": right["rv"]}), "k"), "column 'lv' is on both sides"),
        (lambda: sess.hash_join(left, pa.record_batch({"k": right["k"], "lv": right["rv"]}), "k", join_type="left_outer"), "column 'lv' is on both sides"),
    ]
    for call, text in invalid:
        with pytest.raises(ac.ErrInvalid, match=text):
            call()
    # a name on both sides is no obstacle where the right columns do not come out
    assert sess.hash_join(left, pa.record_batch({"k": right["k"], "lv": right["rv"]}), "k", join_type="left_semi").num_rows > 0
    not_implemented = [
        (lambda: sess.hash_join(left, pa.record_batch({"k": right["k"].cast(pa.int64())}), "k"), "no kernel matching input types"),
        (lambda: sess.hash_join(pa.record_batch({"k": pa.array([b"abc"], pa.binary(3))}), pa.record_batch({"k": pa.array([b"abcd"], pa.binary(4))}), "k"),
         "no kernel matching input types"),
        (lambda: sess.hash_join(pa.record_batch({"k": pa.array([1], pa.decimal128(10, 2))}), pa.record_batch({"k": pa.array([1], pa.decimal128(10, 3))}), "k"),
         "no kernel matching input types"),
        (lambda: sess.hash_join(pa.record_batch({"k": left["ls"].dictionary_encode()}), pa.record_batch({"k": right["rs"].dictionary_encode()}), "k"),
         "dictionary-typed key column 'k'"),
        (lambda: sess.hash_join(left, pa.record_batch({"x": right["rs"].dictionary_encode()}), "ls", "x"), "dictionary-typed key column 'x'"),
    ]
    for call, text in not_implemented:
        with pytest.raises(ac.ErrNotImplemented, match=text):
            call()


@pytest.mark.gpu
def test_a_host_resident_column_never_reaches_the_join():
    """HashJoinImpl refuses host-resident columns (NotImplemented, worded like group_by's refusal), but no caller of the C API can
    hand it one: ahc_record_from_arrays uploads every host-resident column when the record batch is put together.  So the reachable
    behaviour is that such a column joins like any other."""
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    try:
        s.set_option("host_threshold_bytes", 0)   # every flat column imported with import_host stays on the host
        keys = pa.array((np.arange(100, dtype=np.int64) * 7) % 60)
        on_host = s.import_host(keys)
        assert on_host.on_host()
        d = C.c_void_p()
        names = (C.c_char_p * 1)(b"k")
        handles = (C.c_void_p * 1)(on_host.h)
        s._check(ac.lib.ahc_record_from_arrays(s.h, 1, names, handles, C.byref(d)))
        batch = ac.DeviceArray(s, d)
        device = pa.record_batch({"k": pa.array(np.arange(50, dtype=np.int64)), "rv": pa.array(np.arange(50, dtype=np.int32))})
        got = s.call_function("hash_join", [batch, device], "left_keys=k")
        assert got.equals(s.hash_join(pa.record_batch({"k": keys}), device, "k")) and got.num_rows == int((keys.to_numpy() < 50).sum())
        batch.release()
        on_host.release()
    finally:
        s.close()


@pytest.mark.gpu
def test_more_than_2_to_the_30_rows_together_are_refused(sess):
    from arrow_go_amd import compute as ac
    n = 1 << 30
    big = pa.record_batch({"k": pa.Array.from_buffers(pa.bool_(), n, [None, pa.py_buffer(bytes(n // 8))])})
    one = pa.record_batch({"k": pa.array([True])})
    with pytest.raises(ac.ErrInvalid, match="more than 2\\^30"):
        sess.hash_join(big, one, "k", join_type="left_semi")


@pytest.mark.gpu
def test_only_the_float_cases_skip_pyarrow(sess):
    """runs last in this file: every case above went to pyarrow as well, except the two with ±0.0 / NaN keys"""
    assert left_to_the_model <= PYARROW_LEFT_OUT and not (compared_with_pyarrow & PYARROW_LEFT_OUT)
    if {"kind_" + k for k in KEY_KINDS} <= compared_with_pyarrow:   # the whole file ran, not a selection of it
        assert left_to_the_model == PYARROW_LEFT_OUT and len(left_to_the_model) == 2
        assert len(compared_with_pyarrow) >= len(KEY_KINDS) + 9
