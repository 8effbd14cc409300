"""ah_group_m2 / ah_group_variance (csrc/ah_group_agg.hip) through Context, against the host model of tests/group_variance_model.py
(DESIGN.md §3.2).

Per call: the counts are exact; the means are the BYTES of ah_group_sum_typed + ah_group_mean on the column cast to Float64 with numpy;
M2 is within 1 ULP of the model's exact sum of the t_i rounded once (the accumulator's bound: ½ ulp + n_g · 2^−94 · Σ t_i, below 1 ULP
for the 2^30 rows a call takes), NaN for NaN and infinity for infinity.  Every output is pre-filled with 0xA5 and lies between two guard
words, one in front and one behind, which are read back with it."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import group_variance_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow_go_amd", "csrc")
TYPE_IDS = {np.uint8: 2, np.int8: 3, np.uint16: 4, np.int16: 5, np.uint32: 6, np.int32: 7, np.uint64: 8, np.int64: 9, np.float32: 11, np.float64: 12}
ALL = list(TYPE_IDS)
GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)


def source_constant(fname, name):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, fname)).read())
    assert m, (fname, name)
    return int(m.group(1))


STEP = source_constant("ah_hashing.h", "kBlock") * 8          # rows one workgroup takes per step of the skeleton
LDS_GROUPS = source_constant("ah_group_agg.hip", "kTypedLdsGroups")
assert (STEP, LDS_GROUPS) == (2048, 4096)
ROWS = [1, 63, 64, 65, STEP - 1, STEP, STEP + 1, 3 * STEP + 77]
VOFFS = [None, 0, 1, 7, 63, 65]


# ---- no GPU needed ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from arrow_go_amd import _native as N
    from arrow_go_amd import device as D
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    src = open(os.path.join(ROOT, "arrow_go_amd", "device.py")).read()
    go = open(os.path.join(ROOT, "go", "arrowhip", "extra.go")).read()
    for sym, nargs in {"ah_group_m2": 11, "ah_group_variance": 7}.items():
        assert sym in N.declared_symbols() and sym in exported, sym
        assert len(getattr(N.lib, sym).argtypes) == nargs, sym
        assert "lib." + sym in src and "C." + sym + "(" in go, sym
    assert callable(D.Context.group_m2) and callable(D.Context.group_variance)


# ---- one call beside its yardsticks ----------------------------------------------------------------------------------------------------
def pack(bits):
    return np.packbits(np.asarray(bits, bool), bitorder="little")


class Guarded:
    """ng 8-byte slots for a call to write, with a guard word in front and one behind: `out` is what the call gets"""
    def __init__(self, ctx, ng):
        self.ng, self.buf = ng, ctx.alloc((ng + 2) * 8 + 64)
        self.buf.memset(0xA5)
        self.out = self.buf.at(8)

    def words(self):
        raw = self.buf.download(np.uint64, self.ng + 2)
        assert raw[0] == GUARD, "wrote in front of the first group"
        assert raw[self.ng + 1] == GUARD, "wrote past the last group"
        return raw[1:self.ng + 1]

    def read(self):
        w = self.words()
        self.buf.free()
        return w


def guarded(ctx, ng):
    return Guarded(ctx, ng)


def run_m2(ctx, vals, ids, ng, valid=None, voff=0, elem_off=0, seed=0):
    """-> (counts int64, means as uint64 words, m2 as uint64 words) of one ah_group_m2 call"""
    rng = np.random.default_rng(seed)
    w = vals.dtype.itemsize
    ids_b = ctx.to_device(np.asarray(ids, np.int32), 64)
    lead = rng.integers(0, 256, elem_off * w, dtype=np.uint8)
    vals_b = ctx.to_device(np.concatenate([lead, vals.view(np.uint8), rng.integers(0, 256, 8, dtype=np.uint8)]), 64)
    vb = None
    if valid is not None:
        bits = rng.random(voff + len(vals) + 13) < 0.5
        bits[voff:voff + len(vals)] = valid
        vb = ctx.to_device(pack(bits), 64)
    means, m2, counts = guarded(ctx, ng), guarded(ctx, ng), guarded(ctx, ng)
    ctx.group_m2(TYPE_IDS[vals.dtype.type], ids_b, ng, vals_b.ptr + elem_off * w, vb, voff, len(vals), means.out, m2.out, counts.out)
    ctx.sync()
    out = counts.read().view(np.int64), means.read(), m2.read()
    for b in (ids_b, vals_b, vb):
        if b is not None:
            b.free()
    return out


def yardstick_means(ctx, vals, ids, ng, valid):
    """ah_group_sum_typed + ah_group_mean on the column cast to Float64 (AH_FLOAT64 = 12) -> uint64 words"""
    cast = vals.astype(np.float64)
    ids_b, cast_b = ctx.to_device(np.asarray(ids, np.int32), 64), ctx.to_device(cast, 64)
    vb = ctx.to_device(pack(valid), 64) if valid is not None else None
    sums, counts, means = guarded(ctx, ng), guarded(ctx, ng), guarded(ctx, ng)
    ctx.group_sum_typed(12, ids_b, ng, cast_b, vb, 0, len(vals), sums.out, counts.out)
    ctx.group_mean(12, sums.out, counts.out, ng, means.out)
    ctx.sync()
    out = means.read()
    sums.read(), counts.read()
    for b in (ids_b, cast_b, vb):
        if b is not None:
            b.free()
    return out


def same_or_both_nan(got_words, want_words):
    g, w = got_words.view(np.float64), want_words.view(np.float64)
    return (got_words == want_words) | (np.isnan(g) & np.isnan(w))


def check(ctx, vals, ids, ng, valid=None, voff=0, elem_off=0, in_range_ids=True):
    label = f"{vals.dtype} n={len(vals)} ng={ng} voff={voff} elem_off={elem_off}"
    counts, means, m2 = run_m2(ctx, vals, ids, ng, valid, voff, elem_off, seed=len(vals) + ng)
    want_counts, want_means, want_m2 = M.moments(vals, ids, ng, valid)
    assert counts.tolist() == want_counts.tolist(), label
    if in_range_ids and len(vals):   # (the 64-bit sum makes no promise about an id that is not a group's)
        yard = yardstick_means(ctx, vals, ids, ng, valid)
        bad = np.flatnonzero(~same_or_both_nan(means, yard))
        assert bad.size == 0, f"{label}: mean of group {bad[0]}: {means[bad[0]]:#x}, the cast column's {yard[bad[0]]:#x}"
    bad = np.flatnonzero(~same_or_both_nan(means, want_means.view(np.uint64)))
    assert bad.size == 0, f"{label}: mean of group {bad[0]} is not the model's"
    got = m2.view(np.float64)
    with np.errstate(all="ignore"):
        fin = np.isfinite(want_m2)
        assert (np.isnan(got) == np.isnan(want_m2)).all(), label
        assert (got[np.isinf(want_m2)] == want_m2[np.isinf(want_m2)]).all(), label
        err = np.abs(got[fin] - want_m2[fin]) / np.spacing(np.abs(want_m2[fin]))
    print(f"{label}: largest M2 error {err.max() if err.size else 0.0} ULP")
    assert (err <= 1.0).all(), f"{label}: M2 off by {err.max()} ULP"
    return counts, means, m2


def draw(rng, dtype, n):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return rng.normal(0, 1e3, n).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,elem_off", [(np.int8, 3), (np.float64, 0), (np.float32, 1)], ids=["int8+3", "float64", "float32+1"])
def test_row_counts_group_counts_and_bit_offsets(ctx, dtype, elem_off):
    """rows around the lanes of a wave and one workgroup step, and more than one workgroup (3 steps + 77); groups on both sides of the
    LDS regime; validity at every listed bit offset and without a bitmap; a narrow type at element offset 3; group 0 all null"""
    rng = np.random.default_rng(7)
    # the largest row count meets every bit offset (and no bitmap) at every group count; the others take them in turn, the turn shifted
    # by the group count so that no group count keeps to a subset of the offsets
    cases = [(ROWS[-1], ng, voff) for ng in (1, LDS_GROUPS, LDS_GROUPS + 1) for voff in VOFFS]
    cases += [(n, ng, VOFFS[(ri + 2 * gi) % len(VOFFS)]) for ri, n in enumerate(ROWS[:-1]) for gi, ng in enumerate((1, LDS_GROUPS, LDS_GROUPS + 1))]
    for n, ng, voff in cases:
        ids = rng.integers(0, ng, n).astype(np.int32)
        valid = None
        if voff is not None:
            valid = rng.random(n) < 0.85
            if ng > 1:
                valid[ids == 0] = False
        counts, means, m2 = check(ctx, draw(rng, dtype, n), ids, ng, valid, voff or 0, elem_off)
        if valid is not None and ng > 1:
            assert counts[0] == 0 and means[0] == 0 and m2[0] == 0     # no valid value: zero bytes


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ALL, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("ng", [37, LDS_GROUPS + 37])
def test_every_numeric_type(ctx, dtype, ng):
    rng = np.random.default_rng(11)
    n = 2 * STEP + 301
    check(ctx, draw(rng, dtype, n), rng.integers(0, ng, n).astype(np.int32), ng, rng.random(n) < 0.9, voff=5)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int64, np.uint64], ids=lambda d: np.dtype(d).name)
def test_eight_byte_integers_beyond_2_53_take_the_float64_mean(ctx, dtype):
    """values near 2^62 (2^63 + 2^62 unsigned) with low bits that the double drops: a few thousand of them wrap the 64-bit sum, and the
    mean must be the Float64 one all the same"""
    rng = np.random.default_rng(13)
    n, ng = 5000, 3
    base = 2**62 if dtype is np.int64 else 2**63 + 2**62
    vals = np.full(n, base, dtype) + rng.integers(0, 2**20, n).astype(dtype)
    ids = (np.arange(n) % ng).astype(np.int32)
    assert sum(int(v) for v in vals[ids == 0]) >= 2**64
    counts, means, m2 = check(ctx, vals, ids, ng)
    assert (np.abs(means.view(np.float64) - float(base)) < 2.0**21).all()
    check(ctx, vals, ids, ng + LDS_GROUPS, rng.random(n) < 0.7, voff=9)


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [8, LDS_GROUPS + 8])
def test_an_outlier_group_a_constant_group_and_non_finite_groups(ctx, ng):
    rng = np.random.default_rng(17)
    n = 3 * STEP + 5
    ids = rng.integers(0, 8, n).astype(np.int32)
    vals = rng.normal(5, 100, n)
    valid = rng.random(n) < 0.95
    special = []

    def at(g, k):
        special.append(np.flatnonzero(ids == g)[k])
        return special[-1]

    vals[at(0, 3)] = 1e300                                 # squares that overflow next to groups of ordinary values: +inf there only
    vals[ids == 1] = 1234.5                                  # identical values (n · v exact in double): M2 = 0 exactly
    vals[at(2, 0)] = np.inf
    vals[at(3, 1)] = -np.inf
    vals[at(4, 0)], vals[at(4, 5)] = np.inf, -np.inf
    vals[at(5, 2)] = np.nan
    vals[at(6, 0)], vals[at(6, 1)] = 1e120, 3e-200           # a wide group whose squares stay finite: its own scale
    valid[special] = True
    counts, means, m2 = check(ctx, vals, ids, ng, valid, voff=3)
    got = m2.view(np.float64)
    assert got[0] == np.inf and m2[1] == 0 and np.isnan(got[2:6]).all() and np.isfinite(got[6:8]).all() and (got[6:8] > 0).all()
    with np.errstate(over="ignore"):
        f32 = vals.astype(np.float32)                        # the same through Float32: 1e300 is +inf there
    check(ctx, f32, ids, ng, valid, voff=3)


@pytest.mark.gpu
def test_identical_bytes_across_runs_grids_and_regimes(ctx):
    """the grid is min(steps, blocks_per_cu · CUs): 301 steps make the two settings two grids"""
    rng = np.random.default_rng(19)
    n, ng = 300 * STEP + 5, LDS_GROUPS
    ids = rng.integers(0, ng, n).astype(np.int32)
    vals = rng.normal(0, 1e3, n)
    valid = rng.random(n) < 0.8
    a = run_m2(ctx, vals, ids, ng, valid, voff=1)
    b = run_m2(ctx, vals, ids, ng, valid, voff=1)
    ctx.set_option("blocks_per_cu", 1)
    try:
        c = run_m2(ctx, vals, ids, ng, valid, voff=1)
    finally:
        ctx.set_option("blocks_per_cu", 0)
    d = run_m2(ctx, vals, ids, ng + 1, valid, voff=1)        # one more, empty group: the device-atomic regime
    assert d[0][ng] == 0 and d[1][ng] == 0 and d[2][ng] == 0
    for other in (b, c, tuple(x[:ng] for x in d)):
        for name, x, y in zip(("counts", "means", "m2"), a, other):
            assert bytes(x) == bytes(y), name
    i32 = rng.integers(-10**6, 10**6, n).astype(np.int32)    # and an integer column through the exact integer sum
    e, f = run_m2(ctx, i32, ids, ng, valid, voff=1), run_m2(ctx, i32, ids, ng + 1, valid, voff=1)
    assert all(bytes(x) == bytes(y[:ng]) for x, y in zip(e, f))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int16, np.float64], ids=lambda d: np.dtype(d).name)
def test_ids_outside_the_groups_touch_nothing(ctx, dtype):
    rng = np.random.default_rng(23)
    n = 2 * STEP + 9
    for ng in (5, LDS_GROUPS + 904):
        ids = rng.integers(0, ng, n).astype(np.int32)
        ids[::5], ids[1::7], ids[2::11] = -1, ng, 2**31 - 1
        check(ctx, draw(rng, dtype, n), ids, ng, rng.random(n) < 0.9, voff=2, in_range_ids=False)   # (the guard words in front of and behind every output: Guarded)


@pytest.mark.gpu
def test_no_groups_and_no_rows(ctx):
    ids, vals = ctx.alloc(4096), ctx.alloc(4096)
    outs = [guarded(ctx, 4) for _ in range(3)]
    ctx.group_m2(7, ids, 0, vals, None, 0, 100, *[o.out for o in outs])       # no groups: nothing touched
    ctx.group_m2(7, None, 0, None, None, 0, 100, None, None, None)
    ctx.group_variance(None, None, 0, 1, True, None)
    ctx.sync()
    for o in outs:
        assert (o.words() == GUARD).all()
    ctx.group_m2(12, ids, 4, vals, None, 0, 0, *[o.out for o in outs])        # no rows: every group is empty
    ctx.sync()
    for o in outs:
        assert o.read().tolist() == [0, 0, 0, 0]
    ids.free()
    vals.free()


@pytest.mark.gpu
def test_the_finisher_is_one_division_and_one_square_root(ctx):
    rng = np.random.default_rng(29)
    ng = 3000
    counts = rng.integers(0, 10**6, ng).astype(np.int64)
    counts[:40] = np.arange(40) % 5
    m2 = np.abs(rng.normal(0, 1e6, ng)) * rng.choice([1e-300, 1.0, 1e300], ng)
    m2[-4:] = [np.inf, np.nan, 0.0, 5e-324]
    mb, cb = ctx.to_device(m2, 64), ctx.to_device(counts, 64)
    for ddof in (0, 1, 3):
        for take_sqrt in (False, True):
            ob = guarded(ctx, ng)
            ctx.group_variance(mb, cb, ng, ddof, take_sqrt, ob.out)
            ctx.sync()
            got = ob.read()
            want, is_valid = M.finish(m2, counts, ddof, take_sqrt)
            assert (got[~is_valid] == 0).all() and (~is_valid).sum() >= 8
            bad = np.flatnonzero(~same_or_both_nan(got, want.view(np.uint64)))
            assert bad.size == 0, (ddof, take_sqrt, int(bad[0]), got[bad[0]], want[bad[0]])
    mb.free()
    cb.free()


@pytest.mark.gpu
def test_argument_checks(ctx):
    from arrow_go_amd import _native as N
    ids, vals, out = ctx.alloc(4096), ctx.alloc(4096), ctx.alloc(4096)
    out.memset(0xA5)
    calls = [
        (N.ErrInvalid, "negative", lambda: ctx.group_m2(7, ids, 4, vals, None, 0, -1, out, out, out)),
        (N.ErrInvalid, "null buffer", lambda: ctx.group_m2(7, ids, 4, None, None, 0, 8, out, out, out)),
        (N.ErrInvalid, "null buffer", lambda: ctx.group_m2(7, ids, 4, vals, None, 0, 8, out, None, out)),
        (N.ErrNotImplemented, "type id 1 ", lambda: ctx.group_m2(1, ids, 4, vals, None, 0, 8, out, out, out)),
        (N.ErrNotImplemented, "2^30 rows", lambda: ctx.group_m2(7, ids, 4, vals, None, 0, 2**30 + 1, out, out, out)),
        (N.ErrInvalid, "negative ddof", lambda: ctx.group_variance(vals, ids, 4, -1, False, out)),
        (N.ErrInvalid, "null buffer", lambda: ctx.group_variance(vals, None, 4, 0, False, out)),
    ]
    for err, text, call in calls:
        with pytest.raises(err, match=re.escape(text)):
            call()
    ctx.sync()
    assert out.download(np.uint8, 4096).tolist() == [0xA5] * 4096   # no call above launched anything
    for b in (ids, vals, out):
        b.free()
