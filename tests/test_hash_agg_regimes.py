"""Every regime of the id-based hash aggregates (csrc/ah_hash_agg.hip: one kernel skeleton, an aggregate policy each for the Int64 sum,
the fixed-point Float64 sum and min / max) at the smallest shape that reaches it, with option groupby_partition = 0 so that hash_sum
stays on this path.

Sums are compared byte for byte with the oracle (Float64 columns hold integers: every order of addition is exact), min / max with the
restatement of tests/test_hash_min_max.py.  Key validity starts at bit 3, value validity at bit 5; about 5 % of the keys and 10 % of the
values are null; every output starts as 0xA5 bytes."""
import functools
import math

import numpy as np
import pytest

from tests.backends import HipBackend, OracleBackend
from tests.test_hash_min_max import DTYPES, Run, check, model, sliced_bitmap

pytestmark = pytest.mark.gpu
KOFF, VOFF = 3, 5

# regime -> (rows, key pool, a key that owns a third of the rows, groups expected or None, sums only, hash_sum_partition)
SHAPES = {}
for n in (2047, 2048, 2049):                                   # one workgroup step is 256 × 8 rows
    SHAPES[f"row-loop-tail-{n}"] = (n, 299, False, 300, False, 1)
for groups in (4095, 4096, 4097):                              # the LDS table holds 4096 groups (the null key's is one of them)
    SHAPES[f"lds-boundary-{groups}"] = (1 << 16, groups - 1, False, groups, False, 1)
for n in (65535, 65536, 65537, (1 << 17) + 1):                 # keys drawn from 70000: runs of 1024 rows or more; a chunk is 2^16 rows
    SHAPES[f"bucket-walk-{n}"] = (n, 70000, False, None, False, 1)
SHAPES["short-runs"] = ((1 << 19) + 3, 1 << 22, False, None, False, 1)          # nearly distinct keys: runs under 1024 rows at the chunk edges
SHAPES["short-and-long-runs"] = ((1 << 19) + 3, 1 << 22, True, None, False, 1)  # … and one run of a third of the rows: both kinds in one chunk
SHAPES["two-pass-partition"] = ((1 << 20) + (1 << 18) + 5, 0, False, None, True, 1)   # pool 0: all keys distinct, more than 2^20 groups
SHAPES["plain-device-atomics"] = (1 << 16, 4999, False, 5000, True, 0)


@functools.lru_cache(maxsize=2)
def column(regime):
    """-> keys, key bitmap, {kind: values}, value bitmap: one column per regime, shared by the aggregates"""
    n, pool, hot, _, _, _ = SHAPES[regime]
    rng = np.random.default_rng(sum(regime.encode()) + n)
    if pool == 0:
        k, first = rng.permutation(n) + 1, 1
    elif pool <= n:   # every key of the pool occurs, introduced by a row with a valid key
        k, first = np.concatenate([rng.permutation(pool), rng.integers(0, pool, n - pool)]), pool
    else:
        k, first = rng.integers(0, pool, n), 1
    keys = k.astype(np.int64) * 1000003
    keys[keys == keys[0]] = -1                                 # the all-ones key: the tables' EMPTY marker
    if hot:
        keys[first:][rng.random(n - first) < 1 / 3] = 7 * 1000003
    kv = rng.random(n) < 0.95
    kv[:first] = True
    kv[n - 1] = False                                          # (at least one null key)
    vv = rng.random(n) < 0.9
    f = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    f[rng.random(n) < 0.02] = np.nan
    vals = {"sum-i64": rng.integers(-2**62, 2**62, n, dtype=np.int64), "sum-f64": rng.integers(-1000, 1000, n).astype(np.float64),
            "min_max-i64": rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True), "min_max-f64": f}
    return keys, sliced_bitmap(rng, kv, KOFF), vals, sliced_bitmap(rng, vv, VOFF)


@pytest.fixture(scope="module")
def hip(ctx):
    return HipBackend(ctx, dirty_outputs=True)


@pytest.fixture(scope="module")
def orc_be():
    return OracleBackend()


CASES = [(regime, agg) for regime, shape in SHAPES.items() for agg in ("sum-i64", "sum-f64", "min_max-i64", "min_max-f64")
         if agg.startswith("sum") or not shape[4]]


@pytest.mark.parametrize("regime,agg", CASES, ids=[f"{regime}-{agg}" for regime, agg in CASES])
def test_regime(ctx, hip, orc_be, regime, agg):
    n, pool, hot, groups, _, partition = SHAPES[regime]
    entry, kind = agg.split("-")
    keys, kvalid, vals, vvalid = column(regime)
    v = vals[agg]
    try:
        ctx.set_option("groupby_partition", 0)
        ctx.set_option("hash_sum_partition", partition)
        if entry == "sum":
            got = hip.hash_sum(kind, keys, kvalid, KOFF, v, vvalid, VOFF)
        else:
            run = Run(ctx, kind, keys.view(np.uint64), kvalid, KOFF, v.view(DTYPES[kind]), vvalid, VOFF)
    finally:
        ctx.set_option("groupby_partition", 1)
        ctx.set_option("hash_sum_partition", 1)
    if entry == "sum":
        want = orc_be.hash_sum(kind, keys, kvalid, KOFF, v, vvalid, VOFF)
        for name, a, b in zip(("keys", "sums", "counts"), got[:3], want[:3]):
            assert a.tobytes() == b.tobytes(), name
        assert got[3] == want[3] and got[4].tobytes() == want[4].tobytes()      # null group, first rows
        ngroups = got[0].size
    else:
        check(run, model(kind, keys.view(np.uint64), kvalid, KOFF, v, vvalid, VOFF), kind)
        ngroups = run.ngroups
    if groups is not None:
        assert ngroups == groups
    elif pool == 0:
        assert ngroups > 1 << 20
    else:
        assert ngroups > 4096


def test_float64_sums_are_the_correctly_rounded_exact_sums(ctx, hip, orc_be):
    """a column inside 42 binades: one fixed-point scale holds every addend exactly, so each group's sum is the exact sum rounded once
    (the contract stated in ah_hashing.h) — math.fsum of the group's values, whatever their order"""
    n, pool = 70001, 499
    rng = np.random.default_rng(4207)
    keys = np.concatenate([rng.permutation(pool), rng.integers(0, pool, n - pool)]).astype(np.int64) * 1000003
    keys[keys == keys[0]] = -1
    kv, vv = rng.random(n) < 0.95, rng.random(n) < 0.9
    kv[:pool] = True
    kv[n - 1] = False
    v = (1.0 + rng.random(n)) * 2.0 ** rng.integers(-20, 20, n) * rng.choice([-1.0, 1.0], n)      # 40 binades, no two addends alike
    kvalid, vvalid = sliced_bitmap(rng, kv, KOFF), sliced_bitmap(rng, vv, VOFF)
    try:
        ctx.set_option("groupby_partition", 0)
        got = hip.hash_sum("f64", keys, kvalid, KOFF, v, vvalid, VOFF)
    finally:
        ctx.set_option("groupby_partition", 1)
    want = orc_be.hash_sum("f64", keys, kvalid, KOFF, v, vvalid, VOFF)
    assert got[0].size == pool + 1 and got[0].tobytes() == want[0].tobytes() and got[2].tobytes() == want[2].tobytes() and got[3] == want[3]
    rows = {}
    for i in np.flatnonzero(vv):
        rows.setdefault(int(keys[i]) if kv[i] else None, []).append(v[i])
    order = [None if g == got[3] else int(k) for g, k in enumerate(got[0].view(np.int64))]
    exact = np.array([math.fsum(rows.get(k, [])) for k in order], np.float64)
    assert got[1].tobytes() == exact.tobytes()
