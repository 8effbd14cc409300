"""if_else, coalesce, fill_null, fill_null_forward and fill_null_backward through Session against pyarrow (Arrow C++ defines them):
int32, int64 + int32 (the promotion), float64 with NaNs, bool, string and decimal128; array and scalar arguments, a scalar and a
null-scalar condition; sliced inputs (offset 5); chunked arrays whose chunk border falls inside a null run; coalesce with 1, 2 and
4 arguments; coalesce over the null column a left_outer hash_join leaves; an expression tree through the per-call executor; a
keep_on_device round trip.  Results are compared with Array.equals (floats by the bit patterns of their valid rows: NaN is not
equal to NaN for pyarrow), and the library's own rule under null slots — zero payload — on the buffers."""
import decimal

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc  # noqa: E402

pytestmark = pytest.mark.gpu

N = 3001   # several validity words and a partial last byte
TYPES = {"int32": pa.int32(), "float64": pa.float64(), "bool": pa.bool_(), "string": pa.string(), "decimal128": pa.decimal128(20, 3)}


@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.close()


def column(t, n, null_rate, seed, offset=5):
    """n rows of type t at offset `offset` of a longer array"""
    rng = np.random.default_rng(seed)
    total = n + offset
    if pa.types.is_boolean(t):
        vals = (rng.random(total) < 0.5).tolist()
    elif pa.types.is_floating(t):
        x = rng.standard_normal(total)
        x[rng.random(total) < 0.05] = np.nan
        vals = x.tolist()
    elif pa.types.is_integer(t):
        info = np.iinfo(t.to_pandas_dtype())
        vals = rng.integers(info.min, info.max, total, dtype=t.to_pandas_dtype(), endpoint=True).tolist()
    elif pa.types.is_decimal(t):
        vals = [decimal.Decimal(int(v)).scaleb(-3) for v in rng.integers(-10**15, 10**15, total)]
    else:
        vals = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(k))) for k in rng.integers(0, 20, total)]
    mask = rng.random(total) < null_rate
    return pa.array([None if m else v for v, m in zip(vals, mask)], type=t).slice(offset, n)


def same(got, want):
    if isinstance(want, pa.ChunkedArray):
        assert isinstance(got, pa.ChunkedArray) and [len(c) for c in got.chunks] == [len(c) for c in want.chunks]
        for g, w in zip(got.chunks, want.chunks):
            same(g, w)
        return
    assert got.type == want.type and len(got) == len(want), (got.type, want.type, len(got), len(want))
    got.validate(full=True)
    if pa.types.is_floating(got.type):
        assert got.is_valid().equals(want.is_valid())
        got, want = pc.fill_null(got.view(pa.int64()), 0), pc.fill_null(want.view(pa.int64()), 0)
    assert got.equals(want), (got.to_pylist()[:10], want.to_pylist()[:10])


def payload_is_zero_under_nulls(arr):
    if arr.null_count == 0 or pa.types.is_boolean(arr.type) or pa.types.is_string(arr.type) or pa.types.is_large_string(arr.type):
        return
    w = arr.type.bit_width // 8
    rows = np.frombuffer(arr.buffers()[1], np.uint8)[arr.offset * w:(arr.offset + len(arr)) * w].reshape(len(arr), w)
    assert not rows[~np.asarray(arr.is_valid())].any()


@pytest.mark.parametrize("name", list(TYPES))
def test_if_else(sess, name):
    t = TYPES[name]
    cond = column(pa.bool_(), N, 0.1, 1)
    left, right = column(t, N, 0.1, 2), column(t, N, 0.1, 3, offset=69)
    for l, r in ((left, right), (left[3], right), (left, right[4]), (left[3], right[4]), (pa.scalar(None, type=t), right)):
        got = sess.if_else(cond, l, r)
        same(got, pc.if_else(cond, l, r))
        payload_is_zero_under_nulls(got)
    clean = column(pa.bool_(), N, 0.0, 4)
    same(sess.if_else(clean, column(t, N, 0.0, 5), column(t, N, 0.0, 6)), pc.if_else(clean, column(t, N, 0.0, 5), column(t, N, 0.0, 6)))
    # a scalar condition is decided on the host: one side (a scalar side broadcast), or nulls
    for c in (pa.scalar(True), pa.scalar(False), pa.scalar(None, type=pa.bool_())):
        same(sess.if_else(c, left, right), pc.if_else(c, left, right))
        same(sess.if_else(c, left[3], right), pc.if_else(c, left[3], right))
        same(sess.if_else(c, left, right[4]), pc.if_else(c, left, right[4]))


def test_if_else_promotes_numeric_sides(sess):
    cond = column(pa.bool_(), N, 0.1, 1)
    a, b = column(pa.int64(), N, 0.1, 2), column(pa.int32(), N, 0.1, 3)
    want = pc.if_else(cond, a, b.cast(pa.int64()))
    same(sess.if_else(cond, a, b), want)
    same(sess.if_else(cond, b, a), pc.if_else(cond, b.cast(pa.int64()), a))
    same(sess.if_else(cond, a, pa.scalar(7, pa.int32())), pc.if_else(cond, a, pa.scalar(7, pa.int64())))
    same(sess.coalesce(b, a), pc.coalesce(b.cast(pa.int64()), a))
    same(sess.fill_null(b, pa.scalar(-1, pa.int64())), pc.fill_null(b.cast(pa.int64()), pa.scalar(-1, pa.int64())))


def test_refusals_through_the_session(sess):
    from arrow_go_amd import compute as ac
    cond = column(pa.bool_(), 10, 0.1, 1)
    with pytest.raises(ac.ErrNotImplemented, match="no kernel matching"):
        sess.if_else(column(pa.int8(), 10, 0, 1), column(pa.int32(), 10, 0, 2), column(pa.int32(), 10, 0, 3))
    with pytest.raises(ac.ErrNotImplemented, match="no kernel matching"):
        sess.if_else(cond, column(pa.string(), 10, 0, 2), column(pa.int32(), 10, 0, 3))
    with pytest.raises(ac.ErrNotImplemented, match="no kernel matching"):   # one id, other parameters
        sess.if_else(cond, column(pa.decimal128(20, 3), 10, 0, 2), pa.array([decimal.Decimal("1.5")] * 10, pa.decimal128(10, 1)))
    with pytest.raises(ac.ErrInvalid, match="same length"):
        sess.if_else(cond, column(pa.int32(), 10, 0, 2), column(pa.int32(), 11, 0, 3))
    with pytest.raises(ac.ErrInvalid, match="accepts 3 arguments"):
        sess.call_function("if_else", [cond, cond])


@pytest.mark.parametrize("name", list(TYPES))
def test_coalesce_and_fill_null(sess, name):
    t = TYPES[name]
    cols = [column(t, N, rate, 10 + i, offset=(5, 0, 69, 3)[i]) for i, rate in enumerate((0.5, 0.5, 0.5, 0.2))]
    for k in (1, 2, 4):
        got = sess.coalesce(*cols[:k])
        same(got, pc.coalesce(*cols[:k]))
        payload_is_zero_under_nulls(got)
    clean = column(t, N, 0.0, 20)
    same(sess.coalesce(cols[0], clean, cols[1]), pc.coalesce(cols[0], clean, cols[1]))   # the fold ends at the column without nulls
    same(sess.coalesce(clean, cols[0]), clean)
    fill = clean[7]
    same(sess.fill_null(cols[0], fill), pc.fill_null(cols[0], fill))
    same(sess.fill_null(cols[0], cols[1]), pc.coalesce(cols[0], cols[1]))
    same(sess.coalesce(pa.scalar(None, type=t), cols[0], fill), pc.coalesce(pa.scalar(None, type=t), cols[0], fill))
    same(sess.coalesce(cols[0], cols[1], fill), pc.coalesce(cols[0], cols[1], fill))


@pytest.mark.parametrize("name", list(TYPES) + ["int64", "int8", "large_string"])
def test_directed_fills(sess, name):
    t = TYPES.get(name) or {"int64": pa.int64(), "int8": pa.int8(), "large_string": pa.large_string()}[name]
    for rate in (0.1, 0.9, 0.0, 1.0):
        col = column(t, N, rate, 30)
        # (pyarrow 25 fills a SLICED boolean array wrongly: its expectation comes from an unsliced copy of the same rows)
        ref = pa.array(col.to_pylist(), type=t) if pa.types.is_boolean(t) else col
        for fn, want in ((sess.fill_null_forward, pc.fill_null_forward(ref)), (sess.fill_null_backward, pc.fill_null_backward(ref))):
            got = fn(col)
            same(got, want)
            payload_is_zero_under_nulls(got)


@pytest.mark.parametrize("name", ["int32", "string", "bool", "decimal128"])
def test_directed_fills_carry_across_chunk_borders(sess, name):
    t = TYPES[name]
    col = column(t, 700, 0.3, 40, offset=0)
    vals = col.to_pylist()
    for i in list(range(190, 320)) + list(range(0, 10)) + list(range(690, 700)):   # a null run across the borders at 200 and 300,
        vals[i] = None                                                             # and runs at both ends
    whole = pa.array(vals, type=t)
    chunked = pa.chunked_array([whole.slice(0, 200), whole.slice(200, 100), whole.slice(300, 0), whole.slice(300, 400)])
    for fn, ref in ((sess.fill_null_forward, pc.fill_null_forward), (sess.fill_null_backward, pc.fill_null_backward)):
        want = ref(pa.array(vals, type=t))
        got = fn(chunked)
        # one output chunk per span between the input's chunk ends; an empty span gives no chunk, as for every chunked call (tests/test_chunked.py)
        assert isinstance(got, pa.ChunkedArray) and [len(c) for c in got.chunks] == [200, 100, 400]
        same(got.combine_chunks() if got.num_chunks else got, want)
    # chunked arguments of the scalar functions: re-chunked at the union of the arguments' chunk ends
    cond = pa.chunked_array([column(pa.bool_(), 200, 0.1, 1), column(pa.bool_(), 500, 0.1, 2)])
    got = sess.if_else(cond, chunked, whole)
    assert isinstance(got, pa.ChunkedArray) and [len(c) for c in got.chunks] == [200, 100, 400]
    same(got.combine_chunks(), pc.if_else(cond.combine_chunks(), whole, whole))


def test_coalesce_over_the_nulls_of_a_left_outer_join(sess):
    rng = np.random.default_rng(7)
    left = pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 400, 2000).astype(np.int64)), pa.array(np.arange(2000, dtype=np.int32))], names=["k", "a"])
    right = pa.RecordBatch.from_arrays([pa.array(np.arange(0, 400, 2, dtype=np.int64)), pa.array(rng.standard_normal(200)),
                                        pa.array(["r%d" % i for i in range(200)])], names=["k", "x", "s"])
    joined = sess.hash_join(left, right, "k", join_type="left_outer")
    x, s = joined.column("x"), joined.column("s")
    assert x.null_count > 0 and x.null_count == s.null_count
    same(sess.coalesce(x, pa.scalar(0.0)), pc.coalesce(x, pa.scalar(0.0)))
    same(sess.coalesce(s, pa.scalar("none")), pc.coalesce(s, pa.scalar("none")))


def test_expression_tree_runs_call_by_call(sess):
    a, b = column(pa.int64(), N, 0.1, 50), column(pa.int64(), N, 0.1, 51)
    tree = ("call", "if_else", [("call", "greater", [("field", 0), ("field", 1)]), ("field", 0), ("field", 1)])
    got, fused = sess.eval_expression_tree(tree, [a, b])
    assert not fused   # nothing of it is added to the fused kernel
    per_call = sess.if_else(sess.call_function("greater", [a, b]), a, b)
    same(got, per_call)
    same(got, pc.if_else(pc.greater(a, b), a, b))
    tree = ("call", "coalesce", [("field", 0), ("call", "fill_null", [("field", 1), ("lit", pa.scalar(5, pa.int64()))])])
    same(sess.eval_expression_tree(tree, [a, b])[0], pc.coalesce(a, pc.fill_null(b, 5)))


def test_keep_on_device_round_trip(sess):
    cond, a, b = column(pa.bool_(), N, 0.1, 60), column(pa.float64(), N, 0.1, 61), column(pa.float64(), N, 0.1, 62)
    d = sess.if_else(cond, a, b, keep_on_device=True)
    filled = sess.fill_null_forward(d, keep_on_device=True)
    back = sess.coalesce(filled, pa.scalar(0.0))
    same(back, pc.coalesce(pc.fill_null_forward(pc.if_else(cond, a, b)), pa.scalar(0.0)))
    same(d.to_arrow(), pc.if_else(cond, a, b))
    for x in (d, filled):
        x.release()
