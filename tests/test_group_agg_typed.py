"""The aggregates over caller-supplied group ids for value columns of every numeric width (csrc/ah_group_agg.hip: ah_group_sum_typed,
ah_group_min_max_typed, ah_group_count, ah_group_mean), DESIGN.md §3.2.

The yardstick for every type is the existing 64-bit entry point (ah_group_sum_i64 / _f64, ah_group_min_max_i64 / _u64 / _f64) run on the
column cast with numpy to Int64, to UInt64 bit patterns or to Float64: sums, minima, maxima (narrowed back to the input type) and counts
must be EQUAL BYTES.  Every output is pre-filled with 0xA5 and compared one slot past the end as well."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow_go_amd", "csrc")
SYMBOLS = {"ah_group_count": 7, "ah_group_sum_typed": 10, "ah_group_min_max_typed": 11, "ah_group_mean": 6}
TYPE_IDS = {np.uint8: 2, np.int8: 3, np.uint16: 4, np.int16: 5, np.uint32: 6, np.int32: 7, np.uint64: 8, np.int64: 9, np.float32: 11, np.float64: 12}
NARROW = [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.float32]
ALL = NARROW + [np.int64, np.uint64, np.float64]


def source_constant(fname, name):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, fname)).read())
    assert m, (fname, name)
    return int(m.group(1))


STEP = source_constant("ah_hashing.h", "kBlock") * 8          # rows one workgroup takes per step of typed_agg_kernel
LDS_GROUPS = source_constant("ah_group_agg.hip", "kTypedLdsGroups")


# ---- no GPU needed ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from arrow_go_amd import _native as N
    from arrow_go_amd import device as D
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    src = open(os.path.join(ROOT, "arrow_go_amd", "device.py")).read()
    go = open(os.path.join(ROOT, "go", "arrowhip", "extra.go")).read()
    for sym, nargs in SYMBOLS.items():
        assert sym in N.declared_symbols() and sym in exported, sym
        assert getattr(N.lib, sym).argtypes is not None and len(getattr(N.lib, sym).argtypes) == nargs, sym
        assert "lib." + sym in src and "C." + sym + "(" in go, sym
    for name in ("group_count", "group_sum_typed", "group_min_max_typed", "group_mean"):
        assert callable(getattr(D.Context, name))


def test_kernels_have_no_scratch_and_fit_the_lds():
    """every kernel of ah_group_agg.hip compiles for gfx950 with zero scratch bytes and a group segment inside gfx950's 160 KiB; the
    LDS regime of the two-word policies leaves room for two workgroups per CU"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the library under test cannot have been built without it"
    kernels = {}
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "ah_group_agg.s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-S",
                            "--cuda-device-only", "-o", out, os.path.join(CSRC, "ah_group_agg.hip")], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.S):
            p = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
            g = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2))
            kernels[m.group(1)] = (int(p.group(1)), int(g.group(1)))
    mine = {k: v for k, v in kernels.items() if "typed_" in k or "group_mean_kernel" in k}
    # sum and min / max of the seven narrow types and the count in both regimes, the per-group absmax of a wide Float32 column
    assert sum("typed_agg_kernel" in k for k in mine) == 2 * len(NARROW) + 2 * len(NARROW) + 2 + 1 and sum("group_mean_kernel" in k for k in mine) == 3
    assert sum("typed_absmax_kernel" in k for k in mine) == 1 and sum("typed_min_max_finish_kernel" in k for k in mine) == len(NARROW)
    for k, (scratch, lds) in kernels.items():
        assert scratch == 0, f"{k}: {scratch} bytes of scratch"
        assert lds <= 163840, f"{k}: {lds} bytes of LDS"
    for k, (scratch, lds) in mine.items():
        assert lds <= 163840 // 2, f"{k}: {lds} bytes of LDS: two workgroups do not fit a CU"


def test_group_by_is_registered():
    from arrow_go_amd import compute as ac
    assert ac.has_function("group_by")
    assert ac.function_num_kernels("group_by") == 0   # a meta function


# ---- one call of everything, beside the 64-bit yardstick -------------------------------------------------------------------------------
def pack(bits):
    return np.packbits(np.asarray(bits, bool), bitorder="little")


def wide(vals):
    """the column as the 64-bit entry points read it -> (cast column, sum kind, min/max kind)"""
    dt = vals.dtype
    if dt.kind == "f":
        return vals.astype(np.float64), "f64", "f64"
    if dt.kind == "i":
        return vals.astype(np.int64), "i64", "i64"
    return vals.astype(np.uint64), "i64", "u64"


class Outs:
    def __init__(self, ctx, ng, widths):
        self.bufs = [ctx.alloc((ng + 1) * w + 64) for w in widths]
        for b in self.bufs:
            b.memset(0xA5)

    def get(self, i, dtype, ng):
        raw = self.bufs[i].download(np.uint8, (ng + 1) * np.dtype(dtype).itemsize)
        assert bytes(raw[ng * np.dtype(dtype).itemsize:]) == b"\xA5" * np.dtype(dtype).itemsize, "wrote past the last group"
        return raw[:ng * np.dtype(dtype).itemsize]

    def free(self):
        for b in self.bufs:
            b.free()


def run_case(ctx, vals, ids, ng, valid=None, voff=0, elem_off=0, seed=0, yardstick=True):
    """-> dict of byte arrays: sums, counts (of the sum), mins, maxs, mm_counts, count; asserts equality with the 64-bit calls"""
    rng = np.random.default_rng(seed)
    dt = vals.dtype
    n, w = len(vals), dt.itemsize
    ids_b = ctx.to_device(np.asarray(ids, np.int32), 64)
    lead = rng.integers(0, 256, elem_off * w, dtype=np.uint8)
    vals_b = ctx.to_device(np.concatenate([lead, vals.view(np.uint8), rng.integers(0, 256, 8, dtype=np.uint8)]), 64)
    vptr = vals_b.ptr + elem_off * w
    vb = None
    if valid is not None:
        bits = rng.random(voff + n + 13) < 0.5
        bits[voff:voff + n] = valid
        vb = ctx.to_device(pack(bits), 64)
    tid = TYPE_IDS[dt.type]
    o = Outs(ctx, ng, [8, 8, w, w, 8, 8])
    ctx.group_sum_typed(tid, ids_b, ng, vptr, vb, voff, n, o.bufs[0], o.bufs[1])
    ctx.group_min_max_typed(tid, ids_b, ng, vptr, vb, voff, n, o.bufs[2], o.bufs[3], o.bufs[4])
    ctx.group_count(ids_b, ng, vb, voff, n, o.bufs[5])
    ctx.sync()
    got = {"sums": o.get(0, np.uint64, ng), "counts": o.get(1, np.int64, ng), "mins": o.get(2, dt, ng), "maxs": o.get(3, dt, ng),
           "mm_counts": o.get(4, np.int64, ng), "count": o.get(5, np.int64, ng)}
    o.free()
    assert bytes(got["counts"]) == bytes(got["mm_counts"]) == bytes(got["count"]), "the three counts differ"
    if yardstick:
        cast, skind, mkind = wide(vals)
        cast_b = ctx.to_device(cast, 64)
        r = Outs(ctx, ng, [8, 8, 8, 8, 8])
        ctx.group_sum(skind, ids_b, ng, cast_b, vb, voff, n, r.bufs[0], r.bufs[1])
        ctx.group_min_max(mkind, ids_b, ng, cast_b, vb, voff, n, r.bufs[2], r.bufs[3], r.bufs[4])
        ctx.sync()
        want_sums, want_counts = r.get(0, np.uint64, ng), r.get(1, np.int64, ng)
        back = lambda raw: raw.view(cast.dtype).astype(dt).view(np.uint8)   # noqa: E731  the 64-bit result narrowed to the input type
        with np.errstate(invalid="ignore"):
            want_mins, want_maxs = back(r.get(2, cast.dtype, ng)), back(r.get(3, cast.dtype, ng))
        want_mm_counts = r.get(4, np.int64, ng)
        r.free()
        cast_b.free()
        label = f"{dt} n={n} ng={ng} voff={voff} elem_off={elem_off}"
        for name, want in (("sums", want_sums), ("counts", want_counts), ("mins", want_mins), ("maxs", want_maxs), ("mm_counts", want_mm_counts)):
            g, e = got[name].view(np.uint8), np.asarray(want).view(np.uint8)
            bad = np.flatnonzero(g != e)
            assert bad.size == 0, f"{label}: {name} differ at byte {bad[0]} of {g.size}"
    for b in (ids_b, vals_b, vb):
        if b is not None:
            b.free()
    return got


def draw(rng, dtype, n):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.integers(-2000, 2000, n) / 8).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ALL, ids=lambda d: np.dtype(d).name)
def test_every_shape_equals_the_64_bit_call_on_the_cast_column(ctx, dtype):
    """row counts around one workgroup step, group counts on both sides of the LDS regime, a validity bitmap at a bit offset, and a
    group (group 0) whose values are all null"""
    rng = np.random.default_rng(7)
    for n in (0, 1, STEP - 1, STEP, STEP + 1, 3 * STEP + 3):
        for ng in (1, LDS_GROUPS, LDS_GROUPS + 1):
            ids = rng.integers(0, ng, n).astype(np.int32)
            vals = draw(rng, dtype, n)
            valid = rng.random(n) < 0.85
            if ng > 1:
                valid[ids == 0] = False
            got = run_case(ctx, vals, ids, ng, valid, voff=(n + ng) % 8, seed=n + ng)
            counts = got["counts"].view(np.int64)
            assert counts.tolist() == np.bincount(ids[valid], minlength=ng).tolist()
            if ng > 1:   # the all-null group: zero bytes everywhere
                assert counts[0] == 0 and not got["sums"][:8].any() and not got["mins"][:vals.itemsize].any() and not got["maxs"][:vals.itemsize].any()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int16, np.uint16], ids=lambda d: np.dtype(d).name)
def test_bit_offsets_and_element_aligned_pointers(ctx, dtype):
    rng = np.random.default_rng(11)
    n, ng = STEP + 37, 19
    ids = rng.integers(0, ng, n).astype(np.int32)
    vals = draw(rng, dtype, n)
    valid = rng.random(n) < 0.7
    for voff in range(8):
        run_case(ctx, vals, ids, ng, valid, voff=voff, elem_off=(0, 1, 3)[voff % 3], seed=voff)
    for elem_off in (1, 3):
        run_case(ctx, vals, ids, ng, None, elem_off=elem_off)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int8, np.uint16, np.int32, np.float32], ids=lambda d: np.dtype(d).name)
def test_many_groups_take_the_device_atomic_route(ctx, dtype):
    rng = np.random.default_rng(13)
    n, ng = 200_000, 70_000
    ids = rng.integers(0, ng, n).astype(np.int32)
    run_case(ctx, draw(rng, dtype, n), ids, ng, rng.random(n) < 0.85, voff=5)
    run_case(ctx, draw(rng, dtype, n), ids, ng, None)


@pytest.mark.gpu
def test_extreme_columns_are_summed_in_64_bits(ctx):
    n, ng = 5000, 3
    ids = (np.arange(n) % ng).astype(np.int32)
    for dtype, v in ((np.int8, -128), (np.int8, 127), (np.int16, -32768), (np.uint8, 255), (np.uint16, 65535), (np.uint32, 2**32 - 1), (np.int32, -2**31)):
        got = run_case(ctx, np.full(n, v, dtype), ids, ng)
        want = [v * int(c) for c in np.bincount(ids, minlength=ng)]
        assert got["sums"].view(np.int64 if v < 0 else np.uint64).tolist() == want   # not the narrow type's wrap
    # an Int64 column that wraps, a UInt64 column above 2^63
    big = np.full(n, 2**62 + 12345, np.int64)
    got = run_case(ctx, big, ids, ng)
    assert got["sums"].view(np.uint64).tolist() == [((2**62 + 12345) * int(c)) % 2**64 for c in np.bincount(ids, minlength=ng)]
    run_case(ctx, np.full(n, 2**64 - 7, np.uint64), ids, ng)


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [6, LDS_GROUPS + 6])
def test_float32_nan_inf_zero_and_wide_columns(ctx, ng):
    rng = np.random.default_rng(17)
    n = 3 * STEP + 5
    ids = rng.integers(0, ng, n).astype(np.int32)
    vals = draw(rng, np.float32, n)
    vals[ids == 0] = np.nan                                   # a NaN-only group: canonical quiet NaN as min and max, NaN as sum
    vals[ids == 1] = np.where(rng.random((ids == 1).sum()) < 0.5, np.float32(-0.0), np.float32(0.0))   # −0 < +0
    vals[np.flatnonzero(ids == 2)[:1]] = np.inf
    vals[np.flatnonzero(ids == 3)[:1]] = -np.inf
    at4 = np.flatnonzero(ids == 4)
    vals[at4[:1]], vals[at4[1:2]] = np.inf, -np.inf           # both infinities: NaN
    vals[np.flatnonzero(ids == 5)[:1]] = np.float32(1e-45)    # a Float32 denormal is a normal double
    got = run_case(ctx, vals, ids, ng, rng.random(n) < 0.9, voff=3)
    if (ids == 0).any():
        assert got["mins"].view(np.uint32)[0] == 0x7FC00000 and got["maxs"].view(np.uint32)[0] == 0x7FC00000
    # more than 42 binades: the per-group scale route of the fixed-point sum
    vals = draw(rng, np.float32, n)
    vals[::97] = np.float32(1e30)
    vals[1::89] = np.float32(1e-30)
    run_case(ctx, vals, ids, ng, rng.random(n) < 0.9, voff=6)


@pytest.mark.gpu
def test_two_calls_give_identical_bytes(ctx):
    rng = np.random.default_rng(19)
    n, ng = 5 * STEP + 1, 300
    ids = rng.integers(0, ng, n).astype(np.int32)
    vals = rng.normal(0, 1e3, n).astype(np.float32)
    valid = rng.random(n) < 0.8
    a = run_case(ctx, vals, ids, ng, valid, voff=1, seed=1)
    b = run_case(ctx, vals, ids, ng, valid, voff=1, seed=1, yardstick=False)
    for k in a:
        assert bytes(a[k]) == bytes(b[k]), k


@pytest.mark.gpu
def test_no_validity_and_ids_out_of_range_touch_nothing(ctx):
    rng = np.random.default_rng(23)
    n = 2 * STEP + 9
    for ng in (5, LDS_GROUPS + 904):
        ids = rng.integers(0, ng, n).astype(np.int32)
        vals = draw(rng, np.int32, n)
        got = run_case(ctx, vals, ids, ng, None)                        # vvalid = NULL: count_all
        assert got["count"].view(np.int64).tolist() == np.bincount(ids, minlength=ng).tolist()
        # ids outside [0, ngroups): the rows are left out (the 64-bit calls make no such promise above 4096 groups: numpy is the yardstick)
        ids[::5], ids[1::7] = -1, ng
        ok = (ids >= 0) & (ids < ng)
        got = run_case(ctx, vals, ids, ng, None, yardstick=False)
        assert got["count"].view(np.int64).tolist() == np.bincount(ids[ok], minlength=ng).tolist()
        want = np.zeros(ng, np.int64)
        np.add.at(want, ids[ok], vals[ok].astype(np.int64))
        assert got["sums"].view(np.int64).tolist() == want.tolist()


@pytest.mark.gpu
def test_mean_is_the_ieee_quotient(ctx):
    rng = np.random.default_rng(29)
    ng = 1000
    counts = rng.integers(0, 10**6, ng).astype(np.int64)
    counts[::13] = 0
    counts[1] = 2**40 + 1
    cases = ((9, rng.integers(-2**62, 2**62, ng).astype(np.int64)),
             (8, np.concatenate([rng.integers(2**63, 2**64, ng // 2, dtype=np.uint64), rng.integers(0, 2**63, ng - ng // 2, dtype=np.uint64)])),
             (12, np.concatenate([rng.normal(0, 1e6, ng - 4), [np.inf, -np.inf, np.nan, -0.0]])))
    cb = ctx.to_device(counts, 64)
    for tid, sums in cases:
        sb, ob = ctx.to_device(sums, 64), ctx.alloc((ng + 1) * 8)
        ob.memset(0xA5)
        ctx.group_mean(tid, sb, cb, ng, ob)
        ctx.sync()
        got = ob.download(np.uint64, ng + 1)
        with np.errstate(all="ignore"):
            want = np.where(counts == 0, 0.0, sums.astype(np.float64) / np.where(counts == 0, 1, counts).astype(np.float64))
        assert got[ng] == np.uint64(0xA5A5A5A5A5A5A5A5)
        nan = np.isnan(want)   # (IEEE 754 leaves the payload of a propagated NaN open: a NaN for a NaN, every other quotient bit for bit)
        assert np.isnan(got[:ng].view(np.float64)[nan]).all()
        bad = np.flatnonzero((got[:ng] != want.view(np.uint64)) & ~nan)
        assert bad.size == 0, (tid, int(bad[0]), got[bad[0]], want[bad[0]])
        sb.free()
        ob.free()
    cb.free()


@pytest.mark.gpu
def test_argument_checks(ctx):
    from arrow_go_amd import _native as N
    ids, vals, out = ctx.alloc(4096), ctx.alloc(4096), ctx.alloc(4096)
    out.memset(0xA5)
    calls = [
        (N.ErrInvalid, "negative", lambda: ctx.group_count(ids, 4, None, 0, -1, out)),
        (N.ErrInvalid, "negative", lambda: ctx.group_sum_typed(7, ids, 4, vals, None, -1, 8, out, out)),
        (N.ErrInvalid, "negative", lambda: ctx.group_min_max_typed(3, ids, -4, vals, None, 0, 8, out, out, out)),
        (N.ErrInvalid, "null buffer", lambda: ctx.group_count(None, 4, None, 0, 8, out)),
        (N.ErrInvalid, "null buffer", lambda: ctx.group_count(ids, 4, None, 0, 8, None)),
        (N.ErrInvalid, "null buffer", lambda: ctx.group_sum_typed(7, ids, 4, None, None, 0, 8, out, out)),
        (N.ErrInvalid, "null buffer", lambda: ctx.group_sum_typed(11, ids, 4, vals, None, 0, 8, None, out)),
        (N.ErrInvalid, "null buffer", lambda: ctx.group_min_max_typed(5, ids, 4, vals, None, 0, 8, out, None, out)),
        (N.ErrInvalid, "null buffer", lambda: ctx.group_mean(9, None, ids, 4, out)),
        (N.ErrNotImplemented, "type id 1 ", lambda: ctx.group_sum_typed(1, ids, 4, vals, None, 0, 8, out, out)),
        (N.ErrNotImplemented, "type id 13 ", lambda: ctx.group_min_max_typed(13, ids, 4, vals, None, 0, 8, out, out, out)),
        (N.ErrNotImplemented, "type id 11", lambda: ctx.group_mean(11, vals, ids, 4, out)),
        (N.ErrNotImplemented, "2^30 rows", lambda: ctx.group_count(ids, 4, None, 0, 2**30 + 1, out)),
    ]
    for err, text, call in calls:
        with pytest.raises(err, match=re.escape(text)):
            call()
    ctx.group_count(None, 0, None, 0, 8, None)            # no groups: nothing touched, no buffer needed
    ctx.group_sum_typed(7, None, 0, None, None, 0, 8, None, None)
    ctx.group_mean(9, None, None, 0, None)
    ctx.sync()
    assert out.download(np.uint8, 4096).tolist() == [0xA5] * 4096   # no call above launched anything
    for b in (ids, vals, out):
        b.free()
