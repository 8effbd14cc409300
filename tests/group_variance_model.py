"""Host model of the group variance, the yardstick of ah_group_m2 / ah_group_variance and of group_by's variance and
stddev.  It evaluates the definition and nothing else:

  x_i  = the value as a double (numpy's cast: round to nearest even)                  d_i = fl(x_i − m_g)      t_i = fl(d_i · d_i)
  m_g  = S_g / (double)n_g, S_g = the exact sum of the x_i rounded once               M2_g = the exact sum of the t_i rounded once
  variance = M2_g / (double)(n_g − ddof), stddev = its square root, null where n_g ≤ ddof

numpy float64 for x, m, d and t (every operation rounded on its own), fractions.Fraction for the two sums, numpy for the final division
and square root.  A group with a non-finite x or t is left to numpy's own sum, which gives the IEEE answer of any order.

`variant` names a deliberately WRONG model, for the tests that show such a model is caught: "ddof_ignored", "fma" (t never rounded on
its own: acc = fl(d · d + acc) in row order, what a contracted multiply-add computes) and "wrapped_int64_mean" (the mean from the
integer sum modulo 2^64)."""
from fractions import Fraction

import numpy as np


def _round_once(fr):
    try:
        return float(fr)   # int / int division in Python is correctly rounded
    except OverflowError:
        return float("inf") if fr > 0 else float("-inf")


def _exact_sum(a):
    """the sum of the doubles in `a`, rounded once; a non-finite addend: numpy's sum"""
    if not np.isfinite(a).all():
        with np.errstate(all="ignore"):
            return float(np.sum(a))
    return _round_once(sum((Fraction(float(v)) for v in a), Fraction(0)))


def moments(vals, ids, ngroups, valid=None, variant=None):
    """-> (counts int64, means float64, m2 float64), ngroups entries each; rows with an id outside [0, ngroups) or a cleared validity
    bit are left out; an empty group has mean 0.0 and m2 0.0"""
    vals, ids = np.asarray(vals), np.asarray(ids)
    ok = (ids >= 0) & (ids < ngroups)
    if valid is not None:
        ok &= np.asarray(valid, bool)
    x = vals.astype(np.float64)
    counts, means, m2 = np.zeros(ngroups, np.int64), np.zeros(ngroups, np.float64), np.zeros(ngroups, np.float64)
    order = np.argsort(np.where(ok, ids, ngroups), kind="stable")
    bounds = np.searchsorted(np.where(ok, ids, ngroups)[order], np.arange(ngroups + 1))
    for g in range(ngroups):
        rows = order[bounds[g]:bounds[g + 1]]
        n = len(rows)
        counts[g] = n
        if n == 0:
            continue
        xs = x[rows]
        s = _exact_sum(xs)
        if variant == "wrapped_int64_mean" and vals.dtype.kind in "iu":
            w = sum(int(v) for v in vals[rows]) % 2**64
            s = float(w - 2**64 if vals.dtype.kind == "i" and w >= 2**63 else w)
        with np.errstate(all="ignore"):
            m = np.float64(s) / np.float64(n)
            d = xs - m
            t = d * d
        means[g] = m
        if variant == "fma" and np.isfinite(d).all():
            acc = 0.0
            for v in d:
                acc = _round_once(Fraction(float(v)) * Fraction(float(v)) + Fraction(acc))
            m2[g] = acc
        else:
            m2[g] = _exact_sum(t)
    return counts, means, m2


def finish(m2, counts, ddof=0, take_sqrt=False, variant=None):
    """-> (values float64 with 0.0 where counts ≤ ddof, is_valid bool)"""
    m2, counts = np.asarray(m2, np.float64), np.asarray(counts, np.int64)
    if variant == "ddof_ignored":
        ddof = 0
    is_valid = counts > ddof
    with np.errstate(all="ignore"):
        v = m2 / np.where(is_valid, counts - ddof, 1).astype(np.float64)
        if take_sqrt:
            v = np.sqrt(v)
    return np.where(is_valid, v, 0.0), is_valid


def exact_inputs(dtype, rng, ngroups=200, p_null=0.2):
    """The construction on which every intermediate of the definition is exact: `ngroups` groups whose valid counts are drawn from
    {1, 2, 4, 8, 16, 32}, values that are multiples of 16 below 2000 in magnitude (Int8: below 128), null rows mixed in, rows permuted.
    -> (ids int32, values, is_valid bool)"""
    dt = np.dtype(dtype)
    lim = 128 if dt.itemsize == 1 else 2000
    lo = 0 if dt.kind == "u" else -((lim - 1) // 16)
    ids, vals, valid = [], [], []
    for g in range(ngroups):
        n = int(rng.choice([1, 2, 4, 8, 16, 32]))
        nulls = int(rng.binomial(n, p_null))
        ids += [g] * (n + nulls)
        vals += (rng.integers(lo, (lim - 1) // 16, n + nulls, endpoint=True) * 16).tolist()
        valid += [True] * n + [False] * nulls
    perm = rng.permutation(len(ids))
    return np.asarray(ids, np.int32)[perm], np.asarray(vals).astype(dt)[perm], np.asarray(valid, bool)[perm]
