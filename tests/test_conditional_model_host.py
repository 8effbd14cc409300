"""tests/conditional_model.py — the byte-level host model the GPU tests of ah_conditional.hip compare against — pinned against
pyarrow (Arrow C++ defines these functions; arrow-go has none of them): pc.if_else, pc.coalesce, pc.fill_null_forward and
pc.fill_null_backward over int8 … float64, bool, string, large_string and decimal128, null rates 0 / 10 % / 100 %, array and
scalar arguments, sliced inputs.  pyarrow's equality does not look under null slots, so the library's own rule there (zero
payload, data bit 0, length 0) is asserted on the model's bytes directly.  No device."""
import decimal
import itertools

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from tests import conditional_model as CM

N = 517   # not a multiple of 8 or 64
NUMERIC = [pa.int8(), pa.uint8(), pa.int16(), pa.uint16(), pa.int32(), pa.uint32(), pa.int64(), pa.uint64(), pa.float32(), pa.float64()]
TYPES = NUMERIC + [pa.bool_(), pa.string(), pa.large_string(), pa.decimal128(20, 3)]
NULL_RATES = (0.0, 0.1, 1.0)


def random_array(t, n, null_rate, rng, offset=0):
    """n rows of type t behind `offset` rows that a slice cuts away again"""
    total = n + offset
    if pa.types.is_boolean(t):
        vals = (rng.random(total) < 0.5).tolist()
    elif pa.types.is_floating(t):
        vals = rng.standard_normal(total).astype(t.to_pandas_dtype())
        vals[rng.random(total) < 0.05] = np.nan
        vals = vals.tolist()
    elif pa.types.is_integer(t):
        info = np.iinfo(t.to_pandas_dtype())
        vals = rng.integers(info.min, info.max, total, dtype=t.to_pandas_dtype(), endpoint=True).tolist()
    elif pa.types.is_decimal(t):
        vals = [decimal.Decimal(int(v)).scaleb(-3) for v in rng.integers(-10**15, 10**15, total)]
    else:
        vals = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(k))) for k in rng.integers(0, 20, total)]
    mask = rng.random(total) < null_rate if null_rate < 1.0 else np.ones(total, bool)
    arr = pa.array([None if m else v for v, m in zip(vals, mask)], type=t)
    return arr.slice(offset, n)


def buf(b, dtype=np.uint8):
    return None if b is None else np.frombuffer(b, dtype=dtype)


def side_of(x, t):
    """a pyarrow array or scalar → the model's side tuple (a scalar: a one-row array, broadcast)"""
    broadcast = isinstance(x, pa.Scalar)
    arr = pa.array([x.as_py()], type=t) if broadcast else x
    bufs = arr.buffers()
    valid = buf(bufs[0]) if arr.null_count else None
    if pa.types.is_string(t) or pa.types.is_large_string(t):
        ow = 4 if pa.types.is_string(t) else 8
        return (ow, 0, buf(bufs[1], np.int32 if ow == 4 else np.int64), buf(bufs[2]) if bufs[2] is not None else np.zeros(0, np.uint8), valid,
                arr.offset, int(broadcast))
    w = 0 if pa.types.is_boolean(t) else t.bit_width // 8
    return (0, w, None, buf(bufs[1]), valid, arr.offset, int(broadcast))


def to_arrow(t, n, valid, *buffers):
    return pa.Array.from_buffers(t, n, [None if valid is None else pa.py_buffer(valid.tobytes())] + [pa.py_buffer(np.asarray(b).tobytes()) for b in buffers])


def model_if_else(cond_data, cond_valid, cond_off, left, right, n, t):
    """the model's call for type t → (pyarrow array, validity flags, the buffers) and the zero rule checked on the bytes"""
    if pa.types.is_boolean(t):
        data, valid = CM.if_else_boolean(cond_data, cond_valid, cond_off, left, right, n)
        ok = CM.bits(valid, 0, n)
        assert not (CM.bits(data, 0, n) & ~ok).any(), "a null row's data bit is 0"
        return to_arrow(t, n, valid, data), valid, (data,)
    if pa.types.is_string(t) or pa.types.is_large_string(t):
        ow = 4 if pa.types.is_string(t) else 8
        offsets, valid, total = CM.if_else_binary_offsets(cond_data, cond_valid, cond_off, left, right, n, ow)
        data = CM.if_else_binary_data(cond_data, cond_valid, cond_off, left, right, n, offsets)
        ok = CM.bits(valid, 0, n)
        assert offsets[0] == 0 and len(data) == total and (np.diff(offsets)[~ok] == 0).all(), "offsets from 0, a null row has length 0"
        return to_arrow(t, n, valid, offsets, data), valid, (offsets, data)
    values, valid = CM.if_else(cond_data, cond_valid, cond_off, left, right, n)
    w = t.bit_width // 8
    ok = CM.bits(valid, 0, n)
    assert not values.reshape(n, w)[~ok].any(), "the payload under a null slot is zero"
    return to_arrow(t, n, valid, values), valid, (values,)


def assert_same(got, want):
    assert got.type == want.type and len(got) == len(want)
    if pa.types.is_floating(got.type):   # NaN is not equal to NaN for Array.equals: the valid rows' bit patterns instead
        as_int = pa.int32() if got.type == pa.float32() else pa.int64()
        assert got.is_valid().equals(want.is_valid())
        got, want = pc.fill_null(got.view(as_int), 0), pc.fill_null(want.view(as_int), 0)
    assert got.equals(want), (got.type, got.to_pylist()[:8], want.to_pylist()[:8])


@pytest.mark.parametrize("t", TYPES, ids=str)
def test_if_else_matches_pyarrow(t):
    rng = np.random.default_rng(len(str(t)))
    for cond_rate, lrate, rrate in itertools.product(NULL_RATES, NULL_RATES, NULL_RATES):
        for lscalar, rscalar in ((False, False), (True, False), (False, True), (True, True)):
            cond = random_array(pa.bool_(), N, cond_rate, rng, offset=5)
            left = random_array(t, N, lrate, rng, offset=3)
            right = random_array(t, N, rrate, rng, offset=69)
            if lscalar:
                left = left[0]
            if rscalar:
                right = right[7]
            want = pc.if_else(cond, left, right)
            cb = cond.buffers()
            got, _, _ = model_if_else(buf(cb[1]), buf(cb[0]) if cond.null_count else None, cond.offset, side_of(left, t), side_of(right, t), N, t)
            assert_same(got, want)


def model_coalesce(args, t, n):
    """the right fold the host layer runs: coalesce(x1 … xk) = if_else(valid(x1), x1, coalesce(x2 … xk)), cond_valid = None"""
    acc = side_of(args[-1], t)
    for x in reversed(args[:-1]):
        s = side_of(x, t)
        if s[4] is None:    # no nulls on the left: it is the answer (a scalar: broadcast below by the last if_else of the caller)
            acc = s
            continue
        if s[6]:            # a null scalar: the rest is the answer
            continue
        _, valid, bufs = model_if_else(s[4], None, s[5], s, acc, n, t)
        if pa.types.is_string(t) or pa.types.is_large_string(t):
            acc = (s[0] if s[0] else acc[0], 0, bufs[0], bufs[1], valid, 0, 0)
            acc = (4 if pa.types.is_string(t) else 8,) + acc[1:]
        else:
            acc = (0, acc[1], None, bufs[0], valid, 0, 0)
    return acc


def side_to_arrow(side, t, n):
    ow, w, offsets, data, valid, off, broadcast = side
    if broadcast:   # the whole fold came down to one scalar
        ones = np.full((n + 7) // 8, 0xFF, np.uint8)
        return model_if_else(ones, None, 0, side, side, n, t)[0]
    if ow:
        return to_arrow(t, n + off, valid, offsets, data).slice(off, n)
    return to_arrow(t, n + off, valid, data).slice(off, n)


@pytest.mark.parametrize("t", TYPES, ids=str)
def test_coalesce_as_a_fold_of_if_else_matches_pyarrow(t):
    rng = np.random.default_rng(len(str(t)) + 1)
    for k in (1, 2, 4):
        for rates in itertools.islice(itertools.product(NULL_RATES, repeat=k), 0, 27):
            args = [random_array(t, N, r, rng, offset=(5, 0, 69, 3)[i]) for i, r in enumerate(rates)]
            assert_same(side_to_arrow(model_coalesce(args, t, N), t, N), pc.coalesce(*args))
    # scalars: fill_null(values, fill) = coalesce(values, fill); a null scalar in front is skipped
    values = random_array(t, N, 0.1, rng, offset=5)
    fill = random_array(t, 8, 0.0, rng)[3]
    assert_same(side_to_arrow(model_coalesce([values, fill], t, N), t, N), pc.fill_null(values, fill))
    assert_same(side_to_arrow(model_coalesce([pa.scalar(None, type=t), values, fill], t, N), t, N), pc.coalesce(pa.scalar(None, type=t), values, fill))


@pytest.mark.parametrize("direction", (0, 1), ids=("forward", "backward"))
@pytest.mark.parametrize("t", TYPES, ids=str)
def test_directed_fills_match_pyarrow(t, direction):
    rng = np.random.default_rng(len(str(t)) + direction)
    fn = pc.fill_null_backward if direction else pc.fill_null_forward
    for rate, offset in itertools.product(NULL_RATES + (0.9,), (0, 5, 69)):
        arr = random_array(t, N, rate, rng, offset=offset)
        # pyarrow 25 fills a SLICED boolean array wrongly (fill_null_forward of [true, null, …] at offset 5 starts with false): the
        # expectation for booleans comes from an unsliced copy of the same rows; the model still reads the sliced buffers
        want = fn(pa.array(arr.to_pylist(), type=t) if pa.types.is_boolean(t) else arr)
        bufs = arr.buffers()
        valid = buf(bufs[0]) if arr.null_count else None
        idx, ivalid, nulls = CM.fill_null_indices(valid, arr.offset, N, direction)
        assert nulls == want.null_count
        # the indices route: what Take makes of (idx, ivalid)
        take = pa.Array.from_buffers(pa.uint32(), N, [pa.py_buffer(ivalid.tobytes()), pa.py_buffer(idx.tobytes())])
        assert_same(arr.take(take), want)
        assert not idx[~CM.bits(ivalid, 0, N)].any(), "a row without a source holds index 0"
        if not (pa.types.is_boolean(t) or pa.types.is_string(t) or pa.types.is_large_string(t)):   # the fused route
            w = t.bit_width // 8
            values, ovalid, nulls2 = CM.fill_null_directed(w, buf(bufs[1]), valid, arr.offset, N, direction)
            assert nulls2 == nulls and ovalid.tobytes() == ivalid.tobytes()
            assert not values.reshape(N, w)[~CM.bits(ovalid, 0, N)].any(), "the payload under a null slot is zero"
            assert_same(to_arrow(t, N, ovalid if nulls or valid is not None else None, values), want)


def test_tables_worked_out_by_hand():
    cond = pa.array([True, False, None, True])
    left, right = pa.array([1, None, 3, 4], pa.int32()), pa.array([10, 20, 30, None], pa.int32())
    cb = cond.buffers()
    got, _, _ = model_if_else(buf(cb[1]), buf(cb[0]), 0, side_of(left, pa.int32()), side_of(right, pa.int32()), 4, pa.int32())
    assert got.to_pylist() == [1, 20, None, 4]
    col = pa.array([None, 1, None, None, 5, None], pa.int64())
    valid = buf(col.buffers()[0])
    fwd, fvalid, fnulls = CM.fill_null_directed(8, buf(col.buffers()[1]), valid, 0, 6, 0)
    bwd, bvalid, bnulls = CM.fill_null_directed(8, buf(col.buffers()[1]), valid, 0, 6, 1)
    assert to_arrow(pa.int64(), 6, fvalid, fwd).to_pylist() == [None, 1, 1, 1, 5, 5] and fnulls == 1
    assert to_arrow(pa.int64(), 6, bvalid, bwd).to_pylist() == [1, 1, 5, 5, 5, None] and bnulls == 1
    assert CM.fill_null_indices(valid, 0, 6, 0)[0].tolist() == [0, 1, 1, 1, 4, 4]
    assert CM.fill_null_indices(valid, 0, 6, 1)[0].tolist() == [1, 1, 4, 4, 4, 0]


def test_offset_overflow_is_the_models_too():
    side = (4, 0, np.array([0, 1 << 20], np.int32), None, None, 0, 1)
    ones = np.full(512, 0xFF, np.uint8)
    with pytest.raises(CM.OffsetOverflow):
        CM.if_else_binary_offsets(ones, None, 0, side, side, 1 << 12, 4)
    assert CM.if_else_binary_offsets(ones, None, 0, side, side, 1 << 12, 8)[2] == 1 << 32
