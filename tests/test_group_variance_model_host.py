"""The host model of the group variance (tests/group_variance_model.py) pinned without a GPU.

pyarrow is the yardstick where every intermediate of the definition is exact (group_variance_model.exact_inputs: counts that are powers
of two, values that are multiples of 16): there its variance is the exact rational variance rounded once, the model's too, and the two
must be EQUAL, null where n_g ≤ ddof.  Two more inputs pin what the exact construction cannot see — the order of roundings and the
mean of a wrapping Int64 column — against math.fsum and against a value known by hand.  `model_checks` holds all of it as a function
of the model, so that the last test can hand it three deliberately wrong models and see each one caught."""
import functools
import math

import numpy as np
import pytest

from tests import group_variance_model as M

pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc   # noqa: E402

DTYPES = [np.int8, np.uint16, np.int32, np.int64, np.float32, np.float64]


def pyarrow_equality(moments, finish, dtype, ddof):
    rng = np.random.default_rng(100 * np.dtype(dtype).itemsize + ddof)
    ng = 200
    ids, vals, valid = M.exact_inputs(dtype, rng, ng)
    table = pa.table({"k": pa.array(ids), "v": pa.array(vals, mask=~valid)})
    opt = pc.VarianceOptions(ddof=ddof)
    want = table.group_by("k", use_threads=False).aggregate([("v", "variance", opt), ("v", "stddev", opt)]).sort_by("k")
    assert want["k"].to_pylist() == list(range(ng))
    counts, _, m2 = moments(vals, ids, ng, valid)
    assert counts.tolist() == np.bincount(ids[valid], minlength=ng).tolist()
    for name, take_sqrt in (("v_variance", False), ("v_stddev", True)):
        got, is_valid = finish(m2, counts, ddof, take_sqrt)
        w = want[name].combine_chunks()
        assert w.type == pa.float64()
        assert [None if not ok else float(v) for v, ok in zip(got, is_valid)] == w.to_pylist(), (np.dtype(dtype).name, ddof, name)


def rounding_order(moments, finish):
    """random doubles: t_i rounded on its own, the two sums rounded once — math.fsum is the exact sum rounded once"""
    rng = np.random.default_rng(5)
    for _ in range(50):
        x = rng.random(8)
        m = math.fsum(x) / 8.0
        want = math.fsum((v - m) * (v - m) for v in x.tolist())
        counts, means, m2 = moments(x, np.zeros(8, np.int32), 1)
        assert counts[0] == 8 and means[0] == m and m2[0] == want


def int64_mean_is_the_float64_one(moments, finish):
    """four times 2^62: the integer sum is 2^64 = 0 (mod 2^64), the Float64 sum 2^64, the mean 2^62, every deviation 0"""
    counts, means, m2 = moments(np.full(4, 2**62, np.int64), np.zeros(4, np.int32), 1)
    assert counts[0] == 4 and means[0] == 2.0**62 and m2[0] == 0.0
    # beyond 2^53 the value is the rounded double: 2^60 + 1 is 2^60
    counts, means, m2 = moments(np.array([2**60 + 1, 2**60], np.int64), np.zeros(2, np.int32), 1)
    assert means[0] == 2.0**60 and m2[0] == 0.0


def model_checks(moments, finish):
    for dtype in DTYPES:
        for ddof in (0, 1):
            pyarrow_equality(moments, finish, dtype, ddof)
    rounding_order(moments, finish)
    int64_mean_is_the_float64_one(moments, finish)


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_model_equals_pyarrow_where_every_intermediate_is_exact(dtype, ddof):
    pyarrow_equality(M.moments, M.finish, dtype, ddof)


def test_the_model_rounds_every_term_and_each_sum_once():
    rounding_order(M.moments, M.finish)


def test_the_model_takes_the_float64_mean_of_an_int64_column():
    int64_mean_is_the_float64_one(M.moments, M.finish)


def test_non_finite_values_follow_numpy():
    ids = np.array([0, 0, 1, 1, 2, 2, 3, 3], np.int32)
    x = np.array([1.0, np.inf, 2.0, np.nan, 1e200, -1e200, 3.0, 3.0])
    counts, means, m2 = M.moments(x, ids, 4)
    assert np.isinf(means[0]) and np.isnan(m2[0])          # the row of the infinity: inf − inf
    assert np.isnan(means[1]) and np.isnan(m2[1])
    assert means[2] == 0.0 and m2[2] == np.inf             # finite values whose squares overflow
    assert means[3] == 3.0 and m2[3] == 0.0
    v, ok = M.finish(m2, counts, 2, True)
    assert not ok.any() and not v.any()                     # n_g ≤ ddof: 0.0 and not valid


@pytest.mark.parametrize("variant", ["ddof_ignored", "fma", "wrapped_int64_mean"])
def test_a_wrong_model_fails_these_checks(variant):
    model_checks(M.moments, M.finish)
    with pytest.raises(AssertionError):
        model_checks(functools.partial(M.moments, variant=variant), functools.partial(M.finish, variant=variant))
