"""The partition-first group-by's "region too small → once more behind a histogram" retry (csrc/ah_part_driver.h: part_with_retry), for the
one-level driver (gb_cut_aggregate, option groupby_partition 8 = 64 partitions) and the two-level driver (gb2_groupby, option 3 = 2048
partitions), with groupby_reserve 1: one hash_sum call per value type, all five outputs byte for byte against the id-based path
(groupby_partition 0) and run to run.

Inputs (built once, shared by the tests):
  one-level      2^21 + 77 rows over 40 000 keys, the first 2^18 rows holding a hot key in rows 64 … 255 of every 256.  At this size the
                 2^21-row sample reads 64 of every 64 rows, so it SEES the hot key and sizes its region for it: whether the first attempt
                 is void here is left to the sample.
  one-level-8M   the same construction at 2^23 + 77 rows (hot key in the first 2^20), where the sample reads rows g·256 … g·256 + 63 and
                 cannot see it: the hot key's region is sized for the ≈ 4000 sampled rows of its partition and meets 786 432.
  two-level      2^21 + 77 rows over 2^21 keys, one key owning 2 % of them: ≈ 42 000 rows for a child region of 1344.
That the last two attempts MUST be void is arithmetic on the inputs, checked without a GPU (test_retry_inputs) together with the group
counts the oracle finds."""
import functools

import numpy as np
import pytest

from tests.backends import HipBackend, OracleBackend

HOT = 11 * 1000003
CASES = {"one-level": (8, (1 << 21) + 77, 1 << 18), "one-level-8M": (8, (1 << 23) + 77, 1 << 20), "two-level": (3, (1 << 21) + 77, 0)}


@functools.lru_cache(maxsize=None)
def inputs(name):
    mode, n, hidden_rows = CASES[name]
    rng = np.random.default_rng(5150 + n % 1000 + mode)
    if mode == 8:
        keys = rng.integers(0, 40000, n).astype(np.int64) * 1000003
        i = np.arange(n)
        keys[(i % 256 >= 64) & (i < hidden_rows)] = HOT
    else:
        keys = rng.integers(0, 1 << 21, n).astype(np.int64) * 1000003
        keys[rng.random(n) < 0.02] = HOT
    vvalid = np.packbits(rng.random(n + 8) < 0.9, bitorder="little")
    iv = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    fv = (1.0 + rng.random(n)) * np.exp(rng.uniform(-12, 12, n)) * rng.choice([-1.0, 1.0], n)
    for a in (keys, vvalid, iv, fv):
        a.setflags(write=False)
    return mode, keys, vvalid, iv, fv


def partition_of(keys, lp):
    """gb_mix / gb_part of csrc/ah_partition.h"""
    x = keys.view(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(32)
    x *= np.uint64(0xD6E8FEB86659FD93)
    return (x ^ (x >> np.uint64(32))) >> np.uint64(64 - lp)


def test_retry_inputs():
    orc = OracleBackend()
    for name, groups in (("one-level", 40000), ("two-level", None)):
        mode, keys, vvalid, iv, _ = inputs(name)
        e = orc.hash_sum("i64", keys, None, 0, iv, vvalid, 5)
        assert e[0].size == (groups or np.unique(keys).size), name
        assert e[2].sum() == int(np.unpackbits(vvalid, bitorder="little")[5:5 + keys.size].sum()), name   # counts: the rows with a value
    # two-level: every final partition's region holds cap2 rows (gb2_groupby) and the hot key alone brings more
    _, keys, _, _, _ = inputs("two-level")
    n = keys.size
    cap2 = ((n // 2048) * 5 // 4 + 64 + 15) & ~15
    hot_rows = int((keys == HOT).sum())
    assert 0.015 * n < hot_rows < 0.025 * n and hot_rows > 16 * cap2
    assert np.unique(keys).size / 2048 < 1280          # … while its groups fit the partitions' LDS tables: the retry answers, not the id-based path
    # one-level-8M: the region of (the hot key's partition, XCD 0) is sized (S + 6·√(S + 1)) · n / sampled + 64 from its S sampled rows
    # (ah_partition.h 1b); the sample reads 64 rows of every `stride`, XCD 0 takes the first eighth of the 4096-row tiles
    _, keys, _, _, _ = inputs("one-level-8M")
    n = keys.size
    sgroups = min(n // 64, 1 << 15) & ~1
    stride = (n // sgroups) & ~63
    assert stride == 256
    xrows = ((-(-n // 4096) + 7) >> 3) * 4096
    i = np.arange(xrows)
    sampled = keys[:xrows][(i % stride < 64) & (i // stride < sgroups)]
    assert (sampled == HOT).sum() < 64                 # (the hot key is one of the 40 000: the rows that drew it by chance)
    part = partition_of(keys[:xrows], 6)
    hot_part = partition_of(np.array([HOT], np.int64), 6)[0]
    s = int((partition_of(sampled, 6) == hot_part).sum())
    cap = (s + 6 * np.sqrt(s + 1)) * n / (sgroups * 64) + 64
    assert int((part == hot_part).sum()) > 16 * cap
    # one-level: the sample covers the column
    n = inputs("one-level")[1].size
    assert (n // (min(n // 64, 1 << 15) & ~1)) & ~63 == 64


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hash_sum_retry(ctx, name):
    mode, keys, vvalid, iv, fv = inputs(name)
    hip = HipBackend(ctx, dirty_outputs=True)
    try:
        ctx.set_option("groupby_reserve", 1)
        ctx.set_option("groupby_partition", 0)
        base = [hip.hash_sum(k, keys, None, 0, v, vvalid, 5) for k, v in (("i64", iv), ("f64", fv))]
        ctx.set_option("groupby_partition", mode)
        got = [hip.hash_sum(k, keys, None, 0, v, vvalid, 5) for k, v in (("i64", iv), ("f64", fv))]
        again = [hip.hash_sum(k, keys, None, 0, v, vvalid, 5) for k, v in (("i64", iv), ("f64", fv))]
    finally:
        ctx.set_option("groupby_partition", 1)
        ctx.set_option("groupby_reserve", 1)
    for other in (base, again):
        for g, b in zip(got, other):
            for j in (0, 1, 2, 4):
                assert g[j].tobytes() == b[j].tobytes(), (name, j)
            assert g[3] == b[3], name
    if name == "one-level":
        assert got[0][0].size == 40000
