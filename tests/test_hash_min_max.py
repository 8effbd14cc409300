"""Group-by min / max over 8-byte keys (ah_hash_min_max_{i64,u64,f64}).

Expected values come from a restatement in Python — a dict in first-seen order; Float64 ordered by Python's own float comparison with the
sign of a zero as the tie-break, NaN recognised by x != x — and every output slot is compared by its bytes.  pyarrow's group_by is a third
opinion on inputs without mixed-sign zeros (Arrow C++ returns either zero there).  The null group's out_keys slot is whatever
dictionary_encode leaves there: it is compared with ah_hash_sum_i64's, not with the restatement."""
import math
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow_go_amd", "csrc")
SYMBOLS = ("ah_hash_min_max_i64", "ah_hash_min_max_u64", "ah_hash_min_max_f64")
DTYPES = {"i64": np.int64, "u64": np.uint64, "f64": np.float64}
QNAN = 0x7FF8000000000000
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def bits_of(kind, x):
    """the 8 bytes of one result value, as an unsigned integer"""
    return struct.unpack("<Q", struct.pack({"i64": "<q", "u64": "<Q", "f64": "<d"}[kind], x))[0]


def order_key(kind, x):
    return (x, math.copysign(1.0, x)) if kind == "f64" else x      # -0 < +0; integers: Python's own (signed / unsigned) order


def unpack_bits(bitmap, off, n):
    if bitmap is None:
        return [True] * n
    return np.unpackbits(np.asarray(bitmap, np.uint8), bitorder="little")[off:off + n].astype(bool).tolist()


def model(kind, keys, kvalid, koff, vals, vvalid, voff):
    """-> dict(keys, mins, maxs, counts, first_rows: lists; mins / maxs as 8-byte patterns; null_group)"""
    n = len(keys)
    kv, vv = unpack_bits(kvalid, koff, n), unpack_bits(vvalid, voff, n)
    ks, xs = np.asarray(keys, np.uint64).tolist(), np.asarray(vals, DTYPES[kind]).tolist()
    groups = {}                                   # key (None: the null key) -> [first_row, count, min, max]; dicts keep insertion order
    for i in range(n):
        k = ks[i] if kv[i] else None
        g = groups.get(k)
        if g is None:
            g = groups[k] = [i, 0, None, None]
        if not vv[i]:
            continue
        g[1] += 1
        x = xs[i]
        if x != x:                                # NaN: counted, never a minimum or maximum
            continue
        if g[2] is None or order_key(kind, x) < order_key(kind, g[2]):
            g[2] = x
        if g[3] is None or order_key(kind, x) > order_key(kind, g[3]):
            g[3] = x
    out = dict(keys=[], mins=[], maxs=[], counts=[], first_rows=[], null_group=-1)
    for gid, (k, (first, cnt, lo, hi)) in enumerate(groups.items()):
        if k is None:
            out["null_group"] = gid
        out["keys"].append(k)
        out["first_rows"].append(first)
        out["counts"].append(cnt)
        if cnt == 0:
            out["mins"].append(0); out["maxs"].append(0)
        elif lo is None:                          # valid values, all of them NaN
            out["mins"].append(QNAN); out["maxs"].append(QNAN)
        else:
            out["mins"].append(bits_of(kind, lo)); out["maxs"].append(bits_of(kind, hi))
    return out


def test_the_restatement_on_a_table_worked_by_hand():
    nan, inf = float("nan"), float("inf")
    m = model("f64", [3, 3, 4, 3, 4, 5], None, 0, [0.0, -0.0, nan, -inf, nan, 1.0], np.array([0b011111], np.uint8), 0)
    assert m["keys"] == [3, 4, 5] and m["counts"] == [3, 2, 0] and m["first_rows"] == [0, 2, 5] and m["null_group"] == -1
    assert m["mins"] == [0xFFF0000000000000, QNAN, 0] and m["maxs"] == [0x0000000000000000, QNAN, 0]
    m = model("f64", [1, 1], None, 0, [-0.0, 0.0], None, 0)
    assert m["mins"] == [0x8000000000000000] and m["maxs"] == [0]
    m = model("i64", [1, 1, 1], np.array([0b101], np.uint8), 0, [-5, 7, I64_MIN], None, 0)
    assert m["keys"] == [1, None] and m["null_group"] == 1 and m["mins"] == [bits_of("i64", I64_MIN), 7] and m["maxs"] == [bits_of("i64", -5), 7]
    m = model("u64", [1, 1], None, 0, np.array([1 << 63, 5], np.uint64), None, 0)
    assert m["mins"] == [5] and m["maxs"] == [1 << 63]


# ---- no GPU needed ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from arrow_go_amd import _native as N
    from arrow_go_amd import device as D
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for sym in SYMBOLS:
        assert sym in N.declared_symbols() and sym in exported, sym
        assert getattr(N.lib, sym).argtypes is not None and len(getattr(N.lib, sym).argtypes) == 15, sym
    assert callable(D.Context.hash_min_max)
    src = open(os.path.join(ROOT, "arrow_go_amd", "device.py")).read()
    for sym in SYMBOLS:
        assert "lib." + sym in src, sym


def test_kernels_have_no_scratch_and_fit_the_lds():
    """every kernel of ah_hash_agg.hip compiles for gfx950 with zero scratch bytes and a group segment inside gfx950's 160 KiB (read
    from the ISA the way tests/test_cast_decimal.py reads it); the LDS regime's tables are what the declarations state: per group a
    32-bit count and 8 bytes (Int64 sum) or 16 bytes (Float64 sum: 128-bit fixed point; min / max) of aggregate"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the library under test cannot have been built without it"
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "hash_agg.s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-S",
                            "--cuda-device-only", "-o", out, os.path.join(CSRC, "ah_hash_agg.hip")], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(out).read()
    kernels = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        p = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
        g = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2))
        kernels[m.group(1)] = (int(p.group(1)), int(g.group(1)))
    lds_of = lambda *words: sorted(lds for k, (_, lds) in kernels.items() if all(w in k for w in words))
    assert len(lds_of("group_agg_kernel", "MinMax")) == 6                   # {u64, i64, f64} × {LDS table, device atomics}
    assert sum("min_max_finish_kernel" in k for k in kernels) == 3
    assert sum("min_max_init_kernel" in k for k in kernels) == 1
    for k, (scratch, lds) in kernels.items():
        assert scratch == 0, f"{k}: {scratch} bytes of scratch"
        assert lds <= 163840, f"{k}: {lds} bytes of LDS"
    assert lds_of("group_agg_kernel", "MinMax") == [0] * 3 + [4096 * 20] * 3
    # the sums: {LDS table, device atomics} each, and the run-by-run kernel behind the partition (its table + the block-wide count's words)
    assert lds_of("group_agg_kernel", "SumI64") == [0, 4096 * 12]
    assert lds_of("group_agg_kernel", "SumF64") == [0, 4096 * 20]
    assert lds_of("group_agg_kernel", "AbsMax") == [0]                      # the per-group scale of wide Float64 columns: device atomics only
    bucket_i64, bucket_f64 = lds_of("bucket_sum_kernel", "SumI64"), lds_of("bucket_sum_kernel", "SumF64")
    assert len(bucket_i64) == 1 and 4096 * 12 <= bucket_i64[0] <= 4096 * 12 + 1024
    assert len(bucket_f64) == 1 and 4096 * 20 <= bucket_f64[0] <= 4096 * 20 + 1024


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------
def pack(bits):
    return np.packbits(np.asarray(bits, bool), bitorder="little")


def sliced_bitmap(rng, valid_rows, off):
    """a bitmap whose bits off … off + n − 1 are valid_rows, with set bits in front of and behind the slice"""
    n = len(valid_rows)
    bits = rng.random(off + n + 13) < 0.5
    bits[:off] = True
    bits[off + n:off + n + 5] = True
    bits[off:off + n] = valid_rows
    return pack(bits)


class Run:
    """one call on the device; outputs pre-filled with 0xA5 so that an unwritten slot shows"""

    def __init__(self, ctx, kind, keys, kvalid, koff, vals, vvalid, voff, first_rows=True, entry="min_max"):
        keys = np.ascontiguousarray(keys, np.uint64)
        vals = np.ascontiguousarray(vals, DTYPES[kind] if entry == "min_max" else np.int64)
        n = keys.size
        self.bufs = [ctx.to_device(keys, 64), ctx.to_device(vals, 64)]
        kvb = ctx.to_device(kvalid, 64) if kvalid is not None else None
        vvb = ctx.to_device(vvalid, 64) if vvalid is not None else None
        room = (n + 1) * 8 + 64
        outs = {name: ctx.alloc(room) for name in ("keys", "mins", "maxs", "counts", "first_rows")}
        for b in outs.values():
            b.memset(0xA5)
        fr = outs["first_rows"] if first_rows else None
        if entry == "min_max":
            ng, nid = ctx.hash_min_max(kind, self.bufs[0], kvb, koff, self.bufs[1], vvb, voff, n, outs["keys"], outs["mins"], outs["maxs"], outs["counts"], fr)
        else:
            ng, nid = ctx.hash_sum("i64", self.bufs[0], kvb, koff, self.bufs[1], vvb, voff, n, outs["keys"], outs["mins"], outs["counts"], fr)
        ctx.sync()
        self.ngroups, self.null_group = ng, nid
        self.out = {name: b.download(np.uint64, ng + 1) for name, b in outs.items()}     # one slot past the groups: still 0xA5 bytes
        for b in self.bufs + [kvb, vvb] + list(outs.values()):
            if b is not None:
                b.free()

    def raw(self, name):
        return self.out[name][:self.ngroups].tobytes()


def check(run, want, kind):
    assert run.ngroups == len(want["keys"]) and run.null_group == want["null_group"]
    for name in ("mins", "maxs", "counts", "first_rows"):
        exp = np.array(want[name], np.uint64)
        got = run.out[name][:run.ngroups]
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"{kind} {name}: group {bad[0]} of {run.ngroups}: got {int(got[bad[0]]):#018x}, want {int(exp[bad[0]]):#018x}"
    real = [g for g in range(run.ngroups) if g != want["null_group"]]
    assert run.out["keys"][real].tolist() == [want["keys"][g] for g in real]
    for name in ("keys", "mins", "maxs", "counts", "first_rows"):
        assert int(run.out[name][run.ngroups]) == 0xA5A5A5A5A5A5A5A5, f"{name}: wrote past the last group"


def check_pyarrow(kind, keys, kvalid, koff, vals, vvalid, voff, want):
    """the third opinion (inputs without mixed-sign zeros)"""
    import pyarrow as pa
    n = len(keys)
    kmask = ~np.array(unpack_bits(kvalid, koff, n)); vmask = ~np.array(unpack_bits(vvalid, voff, n))
    t = pa.table({"k": pa.array(np.asarray(keys, np.uint64), mask=kmask), "v": pa.array(np.asarray(vals, DTYPES[kind]), mask=vmask)})
    r = t.group_by("k", use_threads=False).aggregate([("v", "min"), ("v", "max"), ("v", "count")])
    theirs = {k: (lo, hi, c) for k, lo, hi, c in zip(r["k"].to_pylist(), r["v_min"].to_pylist(), r["v_max"].to_pylist(), r["v_count"].to_pylist())}
    assert len(theirs) == len(want["keys"])
    for g, k in enumerate(want["keys"]):
        lo, hi, c = theirs[k]
        assert c == want["counts"][g], k
        if c == 0:
            assert lo is None and hi is None
        elif lo != lo:
            assert want["mins"][g] == QNAN and want["maxs"][g] == QNAN and hi != hi
        else:
            assert bits_of(kind, lo) == want["mins"][g] and bits_of(kind, hi) == want["maxs"][g], k


def both(ctx, kind, keys, kvalid, koff, vals, vvalid, voff, pyarrow_too=False):
    want = model(kind, keys, kvalid, koff, vals, vvalid, voff)
    run = Run(ctx, kind, keys, kvalid, koff, vals, vvalid, voff)
    check(run, want, kind)
    if pyarrow_too:
        check_pyarrow(kind, keys, kvalid, koff, vals, vvalid, voff, want)
    return run, want


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["i64", "u64", "f64"])
def test_tiny_table(ctx, kind):
    # row:    0     1     2     3     4     5     6     7
    keys = [50, 0, 50, 70, 0, 90, 70, 90]
    kvalid = pack([1, 0, 1, 1, 0, 1, 1, 1])              # rows 1 and 4: the null key, first seen second
    vals = np.array([4, 8, 2, 9, 1, 6, 3, 5]).astype(DTYPES[kind])
    vvalid = pack([1, 1, 0, 1, 1, 0, 1, 0])              # group 90 (rows 5, 7): every value null
    run, want = both(ctx, kind, keys, kvalid, 0, vals, vvalid, 0, pyarrow_too=True)
    assert want["null_group"] == 1 and want["counts"] == [1, 2, 2, 0] and want["first_rows"] == [0, 1, 3, 5]
    assert want["mins"] == [bits_of(kind, v) for v in vals[[0, 4, 6]]] + [0]
    assert want["maxs"] == [bits_of(kind, v) for v in vals[[0, 1, 3]]] + [0]
    # one row: valid, null value, null key
    for kv, vv in ((None, None), (None, pack([0])), (pack([0]), None)):
        both(ctx, kind, [7], kv, 0, vals[:1], vv, 0)
    # no rows: no groups, nothing touched
    outs = [ctx.alloc(64) for _ in range(5)]
    for b in outs:
        b.memset(0xA5)
    assert ctx.hash_min_max(kind, None, None, 0, None, None, 0, 0, *outs) == (0, -1)
    ctx.sync()
    for b in outs:
        assert b.download(np.uint8, 64).tolist() == [0xA5] * 64
        b.free()


@pytest.mark.gpu
def test_float64_specials(ctx):
    nan, inf = float("nan"), float("inf")
    neg_nan = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000123))[0]       # sign set, a payload
    sig_nan = struct.unpack("<d", struct.pack("<Q", 0x7FF0000000000001))[0]
    den = 5e-324
    rows = [(1, nan), (1, 3.5), (1, -2.0), (1, nan),         # NaN mixed with numbers
            (2, nan), (2, neg_nan), (2, sig_nan),            # all NaN
            (3, -0.0), (3, 0.0),                             # {-0, +0} in both orders
            (4, 0.0), (4, -0.0),
            (5, inf), (5, 1e308), (5, -inf), (5, neg_nan),   # ±inf take part
            (6, den), (6, -den), (6, 2 * den), (6, 0.0),     # denormals around zero
            (7, neg_nan), (7, -1.0),                         # a negative NaN must not become the minimum
            (8, -0.0), (9, 0.0), (10, -den), (11, inf), (12, -inf)]
    keys = [k for k, _ in rows]
    vals = np.array([v for _, v in rows], np.float64)
    vals.view(np.uint64)[5] = 0xFFF8000000000123             # (a list → array round trip may quieten or re-sign a NaN: set the bits)
    vals.view(np.uint64)[6] = 0x7FF0000000000001
    vals.view(np.uint64)[14] = vals.view(np.uint64)[19] = 0xFFF8000000000123
    run, want = both(ctx, "f64", keys, None, 0, vals, None, 0)
    f = lambda x: bits_of("f64", x)
    assert want["counts"] == [4, 3, 2, 2, 4, 4, 2, 1, 1, 1, 1, 1]
    assert want["mins"] == [f(-2.0), QNAN, f(-0.0), f(-0.0), f(-inf), f(-den), f(-1.0), f(-0.0), f(0.0), f(-den), f(inf), f(-inf)]
    assert want["maxs"] == [f(3.5), QNAN, f(0.0), f(0.0), f(inf), f(2 * den), f(-1.0), f(-0.0), f(0.0), f(-den), f(inf), f(-inf)]
    # the same rows many times over, shuffled, beyond the LDS regime's warm-up and through the device-atomic regime (5000 more keys)
    rng = np.random.default_rng(5)
    rep = rng.permutation(np.repeat(np.arange(len(rows)), 300))
    k2 = np.concatenate([np.array(keys, np.uint64)[rep], np.arange(100, 5100, dtype=np.uint64)])
    v2 = np.concatenate([vals[rep], rng.standard_normal(5000)])
    for k, v in ((k2[:len(rep)], v2[:len(rep)]), (k2, v2)):
        run, want = both(ctx, "f64", k, None, 0, v, None, 0)
        order = {int(key): g for g, key in enumerate(want["keys"])}
        assert want["mins"][order[3]] == f(-0.0) and want["maxs"][order[3]] == f(0.0) and want["mins"][order[2]] == QNAN
    # without the zeros of mixed sign pyarrow agrees
    keep = np.array([k not in (3, 4, 6) for k in keys])
    both(ctx, "f64", np.array(keys)[keep], None, 0, vals[keep], None, 0, pyarrow_too=True)


@pytest.mark.gpu
def test_integer_extremes(ctx):
    keys = [1, 1, 1, 2, 2, 2, 3, 3]
    iv = np.array([I64_MAX, I64_MIN, 0, -5, -9, -1, I64_MIN, I64_MIN], np.int64)
    run, want = both(ctx, "i64", keys, None, 0, iv, None, 0, pyarrow_too=True)
    assert want["mins"] == [bits_of("i64", I64_MIN), bits_of("i64", -9), bits_of("i64", I64_MIN)]
    assert want["maxs"] == [bits_of("i64", I64_MAX), bits_of("i64", -1), bits_of("i64", I64_MIN)]
    uv = np.array([(1 << 63) + 5, (1 << 63) - 5, 7, 0, (1 << 64) - 1, 1 << 63, (1 << 64) - 1, (1 << 64) - 1], np.uint64)
    run, want = both(ctx, "u64", keys, None, 0, uv, None, 0, pyarrow_too=True)
    assert want["mins"] == [7, 0, (1 << 64) - 1] and want["maxs"] == [(1 << 63) + 5, (1 << 64) - 1, (1 << 64) - 1]
    # the same bytes read as the other kind give other answers: signed order ≠ unsigned order
    run_i, want_i = both(ctx, "i64", keys, None, 0, uv.view(np.int64), None, 0)
    assert want_i["mins"][0] == (1 << 63) + 5 and want_i["maxs"][0] == (1 << 63) - 5
    # many groups (the device-atomic regime) of values around both wrap points
    rng = np.random.default_rng(11)
    n, card = 20000, 6000
    k = rng.integers(0, card, n).astype(np.uint64)
    u = (rng.integers(-1000, 1000, n).astype(np.int64).view(np.uint64) + np.where(rng.random(n) < 0.5, np.uint64(1 << 63), np.uint64(0))).astype(np.uint64)
    both(ctx, "u64", k, None, 0, u, None, 0, pyarrow_too=True)
    both(ctx, "i64", k, None, 0, u.view(np.int64), None, 0, pyarrow_too=True)


def random_case(seed, kind, n, card, null_keys=True):
    rng = np.random.default_rng(seed)
    # every one of the `card` keys occurs when n ≥ card; scattered 64-bit patterns, the all-ones key among them
    k = np.concatenate([rng.permutation(card), rng.integers(0, card, max(n - card, 0))])[:n].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    k[k == k[0]] = np.uint64(0xFFFFFFFFFFFFFFFF)
    if kind == "f64":
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
        v[rng.random(n) < 0.02] = np.nan
        v[v == 0] = 1.0
    else:
        v = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True).view(DTYPES[kind])
    kv = rng.random(n) < 0.97 if null_keys else np.ones(n, bool)
    kv[:card] = True                              # (the rows that introduce the keys: a null there could take a key away)
    vv = rng.random(n) < 0.9
    return rng, k, kv, v, vv


EDGES = [(1, 1 << 16), (4095, 1 << 16), (4096, 1 << 16), (4097, 1 << 16), ((1 << 13) + 1, 1 << 16), (1 << 17, 1 << 18)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["i64", "f64"])
@pytest.mark.parametrize("card,n", EDGES, ids=[f"{c}-groups" for c, _ in EDGES])
def test_regime_edges(ctx, kind, card, n):
    """the LDS table holds 4096 groups: 4095 / 4096 keys (without null keys: exactly that many groups; with them one more — both sides
    of the edge from one key count) and 4097, 2^13 + 1, 2^17 keys in the device-atomic regime (no two-pass partition route is built)"""
    for null_keys in (False, True) if card <= 4097 else (True,):
        rng, k, kv, v, vv = random_case(card * 2 + null_keys, kind, n, card, null_keys)
        run, want = both(ctx, kind, k, pack(kv) if null_keys else None, 0, v, pack(vv), 0, pyarrow_too=kind == "f64" or not null_keys)
        assert run.ngroups == card + (1 if null_keys else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["u64", "f64"])
@pytest.mark.parametrize("card", [300, 5000])
def test_row_counts_around_the_tile(ctx, kind, card):
    """a workgroup's step is 8 · 256 rows"""
    for k_tiles in (1, 3):
        for d in (-1, 0, 1):
            n = 8 * 256 * k_tiles + d
            rng, k, kv, v, vv = random_case(n, kind, n, min(card, n))
            both(ctx, kind, k, pack(kv), 0, v, pack(vv), 0, pyarrow_too=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["i64", "f64"])
def test_slices(ctx, kind):
    n = 3001
    for koff in range(8):
        voff = (koff + 3) % 8
        for card in (40, 4500) if koff in (0, 5) else (40,):
            rng, k, kv, v, vv = random_case(100 + koff, kind, n, min(card, n))
            both(ctx, kind, k, sliced_bitmap(rng, kv, koff), koff, v, sliced_bitmap(rng, vv, voff), voff)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["i64", "f64"])
@pytest.mark.parametrize("others", [50, 6000])
def test_hot_key(ctx, kind, others):
    """one group owns 90 % of 2^18 rows; its extremes sit at the first and the very last row — a look before the atomic that trusted a
    stale slot, or skipped the atomic on a tie it should not, loses exactly these"""
    n = 1 << 18
    rng = np.random.default_rng(others)
    k = np.where(rng.random(n) < 0.9, np.uint64(77), rng.integers(1000, 1000 + others, n).astype(np.uint64))
    k[0] = k[n - 1] = 77
    v = rng.integers(-10**6, 10**6, n).astype(DTYPES[kind])
    for first, last in ((10**7, -10**7), (-10**7, 10**7)):
        v[0], v[n - 1] = first, last
        run, want = both(ctx, kind, k, None, 0, v, None, 0)
        assert want["keys"][0] == 77 and {want["mins"][0], want["maxs"][0]} == {bits_of(kind, v[0]), bits_of(kind, v[n - 1])}


@pytest.mark.gpu
@pytest.mark.parametrize("card", [700, 9000])
def test_groups_are_those_of_hash_sum(ctx, card):
    n = 50001
    rng, k, kv, v, vv = random_case(card, "i64", n, card)
    kb, vb = sliced_bitmap(rng, kv, 3), sliced_bitmap(rng, vv, 6)
    ref = Run(ctx, "i64", k, kb, 3, v, vb, 6, entry="sum")
    for kind in ("i64", "u64", "f64"):
        got = Run(ctx, kind, k, kb, 3, v.view(DTYPES[kind]), vb, 6)
        assert (got.ngroups, got.null_group) == (ref.ngroups, ref.null_group) and ref.null_group >= 0
        for name in ("keys", "counts", "first_rows"):
            assert got.raw(name) == ref.raw(name), (kind, name)
    # out_first_rows is optional
    lean = Run(ctx, "i64", k, kb, 3, v, vb, 6, first_rows=False)
    assert lean.raw("keys") == ref.raw("keys") and lean.raw("counts") == ref.raw("counts")
    assert lean.out["first_rows"].tobytes() == b"\xa5" * (8 * (lean.ngroups + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["i64", "u64", "f64"])
def test_two_calls_give_the_same_bytes(ctx, kind):
    for card in (1000, 20000):
        rng, k, kv, v, vv = random_case(card + 1, kind, 1 << 16, card)
        a = Run(ctx, kind, k, pack(kv), 0, v, pack(vv), 0)
        b = Run(ctx, kind, k, pack(kv), 0, v, pack(vv), 0)
        for name in ("keys", "mins", "maxs", "counts", "first_rows"):
            assert a.out[name].tobytes() == b.out[name].tobytes(), (card, name)
        check(a, model(kind, k, pack(kv), 0, v, pack(vv), 0), kind)


@pytest.mark.gpu
def test_argument_checks(ctx):
    from arrow_go_amd import _native as N
    bufs = [ctx.alloc(256) for _ in range(7)]
    k, v, ok, lo, hi, cnt, fr = bufs
    for kind in ("i64", "u64", "f64"):
        with pytest.raises(N.ErrInvalid, match="hash_min_max: negative length/offset"):
            ctx.hash_min_max(kind, k, None, -1, v, None, 0, 4, ok, lo, hi, cnt, fr)
        with pytest.raises(N.ErrInvalid, match="hash_min_max: negative length/offset"):
            ctx.hash_min_max(kind, k, None, 0, v, None, 0, -4, ok, lo, hi, cnt, fr)
        with pytest.raises(N.ErrInvalid, match="hash_min_max: null buffer"):
            ctx.hash_min_max(kind, k, None, 0, v, None, 0, 4, ok, lo, None, cnt, fr)
        with pytest.raises(N.ErrInvalid, match="hash_min_max: null buffer"):
            ctx.hash_min_max(kind, k, None, 0, None, None, 0, 4, ok, lo, hi, cnt, fr)
    with pytest.raises(ValueError):
        ctx.hash_min_max("f32", k, None, 0, v, None, 0, 4, ok, lo, hi, cnt, fr)
    for b in bufs:
        b.free()
