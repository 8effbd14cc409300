"""Group ids of a tuple of key columns (ah_group_ids) and the aggregates over caller-supplied ids (ah_group_sum_*, ah_group_min_max_*),
DESIGN.md §3.2.

Expected values come from a restatement in Python: a dict keyed by tuples (None for a null; bytes for a string or a fixed slot, a bool for
a Boolean), insertion order = first-seen order.  Every output is pre-filled with 0xA5 and compared by its bytes, one slot past the end
included.  n <= 2^17 everywhere: the dict is the slow part."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow_go_amd", "csrc")
SYMBOLS = {"ah_group_ids": 7, "ah_group_sum_i64": 9, "ah_group_sum_f64": 9, "ah_group_min_max_i64": 10, "ah_group_min_max_u64": 10,
           "ah_group_min_max_f64": 10}
A5_32, A5_64 = np.uint32(0xA5A5A5A5), np.uint64(0xA5A5A5A5A5A5A5A5)


def source_constant(fname, name):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, fname)).read())
    assert m, (fname, name)
    return int(m.group(1))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def model(columns, n):
    """columns: per key column its n keys (None: null) -> (ids, first_rows)"""
    groups, ids, first = {}, [], []
    for i, t in enumerate(zip(*columns) if n else ()):
        g = groups.get(t)
        if g is None:
            g = groups[t] = len(groups)
            first.append(i)
        ids.append(g)
    return ids, first


def test_the_restatement_on_a_table_worked_by_hand():
    a = [b"\1", None, None, b"\1", None, b"\1", None]
    b = [b"a", b"a", b"b", None, None, b"a", b"a"]
    assert model([a, b], 7) == ([0, 1, 2, 3, 4, 0, 1], [0, 1, 2, 3, 4])
    assert model([a], 7) == ([0, 1, 1, 0, 1, 0, 1], [0, 1])
    assert model([[b"ab", b"a", b"abc", b""], [b"c", b"bc", b"", None]], 4) == ([0, 1, 2, 3], [0, 1, 2, 3])   # no concatenation; "" is not null
    assert model([[True, False, True], [b"x", b"x", b"x"]], 3) == ([0, 1, 0], [0, 1])
    assert model([[], []], 0) == ([], [])


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
    for name in ("group_ids", "group_sum", "group_min_max"):
        assert callable(getattr(D.Context, name))
    assert [f[0] for f in D.GroupKey._fields_] == ["offset_width", "byte_width", "bits", "offsets", "data", "valid", "off"]


def test_kernels_have_no_scratch_and_fit_the_lds():
    """every kernel of ah_group_keys.hip, and the TupleKeys instantiations of insert_kernel in ah_hash.hip, compile for gfx950 with zero
    scratch bytes and a group segment inside gfx950's 160 KiB (read from the ISA the way tests/test_hash_min_max.py reads it)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the library under test cannot have been built without it"
    kernels = {}
    with tempfile.TemporaryDirectory() as d:
        for unit in ("ah_group_keys", "ah_hash"):
            out = os.path.join(d, unit + ".s")
            r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-S",
                                "--cuda-device-only", "-o", out, os.path.join(CSRC, unit + ".hip")], capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stderr[-2000:]
            for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.S):
                p = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
                g = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2))
                kernels[(unit, m.group(1))] = (int(p.group(1)), int(g.group(1)))
    mine = {k: v for k, v in kernels.items() if k[0] == "ah_group_keys" or "TupleKeys" in k[1]}
    assert sum("pack_kernel" in k[1] for k in mine) == 1
    assert sorted(re.search(r"TupleKeysILi(\d+)E", k[1]).group(1) for k in mine if "TupleKeys" in k[1]) == ["2", "4", "8"]
    for k, (scratch, lds) in mine.items():
        assert scratch == 0, f"{k}: {scratch} bytes of scratch"
        assert lds <= 163840, f"{k}: {lds} bytes of LDS"


# ---- key columns as Arrow lays them out ---------------------------------------------------------------------------------------------
def pack(bits):
    return np.packbits(np.asarray(bits, bool), bitorder="little")


class Col:
    """one key column on the host.  kind "str" / "large" (payload: a list of bytes), "fixed" (payload: an (n, w) uint8 array) or "bool"
    (payload: a list of bools); the payload is what the buffers hold, under a null too.  valid: None (no validity buffer) or n bools.
    Row i of the call is element off + i: upload() puts `off` junk rows in front and junk behind, in the validity bits as well."""

    def __init__(self, kind, payload, valid=None, off=0):
        self.kind, self.valid, self.off = kind, (None if valid is None else np.asarray(valid, bool)), off
        self.payload = np.ascontiguousarray(payload, np.uint8) if kind == "fixed" else list(payload)
        self.n = len(self.payload)
        self.w = self.payload.shape[1] if kind == "fixed" else 0
        self.bufs = []

    def keys(self):
        if self.kind == "fixed":
            raw, w = self.payload.tobytes(), self.w
            vals = [raw[i * w:(i + 1) * w] for i in range(self.n)]
        elif self.kind == "bool":
            vals = [bool(x) for x in self.payload]
        else:
            vals = [bytes(x) for x in self.payload]
        if self.valid is None:
            return vals
        return [v if ok else None for v, ok in zip(vals, self.valid.tolist())]

    def _bits(self, rng, rows):
        bits = rng.random(self.off + self.n + 13) < 0.5
        bits[self.off:self.off + self.n] = rows
        return pack(bits)

    def upload(self, ctx, rng):
        """-> the descriptor tuple of Context.group_ids"""
        off, n = self.off, self.n
        vb = None
        if self.valid is not None:
            vb = ctx.to_device(self._bits(rng, self.valid), 64)
        if self.kind in ("str", "large"):
            lead = [rng.bytes(int(rng.integers(1, 5))) for _ in range(off)]
            rows = lead + self.payload + [b"tail", b"junk"]
            dt = np.int32 if self.kind == "str" else np.int64
            offsets = (3 + np.concatenate([[0], np.cumsum([len(r) for r in rows])])).astype(dt)
            data = np.frombuffer(b"xyz" + b"".join(rows) + b"!", np.uint8)
            ob, db = ctx.to_device(offsets, 64), ctx.to_device(data, 64)
            self.bufs = [ob, db, vb]
            return (dt().itemsize, 0, 0, ob, db, vb, off)
        if self.kind == "fixed":
            slots = np.concatenate([rng.integers(0, 256, (off, self.w), dtype=np.uint8), self.payload, rng.integers(0, 256, (2, self.w), dtype=np.uint8)])
            db = ctx.to_device(slots, 64)
            self.bufs = [db, vb]
            return (0, self.w, 0, None, db, vb, off)
        db = ctx.to_device(self._bits(rng, np.asarray(self.payload, bool)), 64)
        self.bufs = [db, vb]
        return (0, 0, 1, None, db, vb, off)

    def free(self):
        for b in self.bufs:
            if b is not None:
                b.free()
        self.bufs = []


def strings(values, large=False, off=0, under_null=b""):
    """values: bytes or None per row"""
    valid = None if all(v is not None for v in values) else [v is not None for v in values]
    return Col("large" if large else "str", [under_null if v is None else v for v in values], valid, off)


def numbers(arr, valid=None, off=0):
    a = np.ascontiguousarray(arr)
    return Col("fixed", a.view(np.uint8).reshape(a.size, a.dtype.itemsize), valid, off)


def slots(arr2d, valid=None, off=0):
    return Col("fixed", arr2d, valid, off)


def bools(values, valid=None, off=0):
    return Col("bool", values, valid, off)


class Run:
    """one ah_group_ids call; outputs pre-filled with 0xA5 so that an unwritten or overwritten slot shows"""

    def __init__(self, ctx, cols, n, seed=0, keep=False):
        rng = np.random.default_rng(seed)
        descs = [c.upload(ctx, rng) for c in cols]
        self.ids_buf, self.first_buf = ctx.alloc((n + 1) * 4 + 64), ctx.alloc((n + 2) * 8 + 64)
        self.ids_buf.memset(0xA5)
        self.first_buf.memset(0xA5)
        self.n = n
        self.ngroups = ctx.group_ids(descs, n, self.ids_buf, self.first_buf)
        ctx.sync()
        self.ids = self.ids_buf.download(np.uint32, n + 1)
        self.first = self.first_buf.download(np.uint64, self.ngroups + 1)
        for c in cols:
            c.free()
        if not keep:
            self.free()

    def free(self):
        self.ids_buf.free()
        self.first_buf.free()


def check(run, cols):
    n = run.n
    want_ids, want_first = model([c.keys() for c in cols], n)
    assert run.ngroups == len(want_first), f"{run.ngroups} groups, want {len(want_first)}"
    got, exp = run.ids[:n], np.array(want_ids, np.uint32)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"ids: row {bad[0]} of {n}: got {int(got[bad[0]])}, want {int(exp[bad[0]])}"
    got, exp = run.first[:run.ngroups], np.array(want_first, np.uint64)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"first rows: group {bad[0]} of {run.ngroups}: got {int(got[bad[0]])}, want {int(exp[bad[0]])}"
    assert run.ids[n] == A5_32, "ids: wrote past the last row"
    assert run.first[run.ngroups] == A5_64, "first rows: wrote past the last group"
    return want_ids, want_first


def both(ctx, cols, seed=0):
    n = cols[0].n
    assert all(c.n == n for c in cols)
    run = Run(ctx, cols, n, seed)
    check(run, cols)
    return run


def drawn(rng, pool, n):
    """n rows drawn from `pool` (a list of values, or the rows of an array)"""
    pick = rng.integers(0, len(pool), n)
    return pool[pick] if isinstance(pool, np.ndarray) else [pool[j] for j in pick]


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_by_hand(ctx):
    # (Int32, String): the four null combinations are four groups
    a = numbers(np.array([1, 5, 6, 1, 7, 1, 8, 9], np.int32), valid=[1, 0, 0, 1, 0, 1, 0, 0])
    b = strings([b"a", b"a", b"b", None, None, b"a", b"a", b"b"])
    run = both(ctx, [a, b])
    assert run.ids[:8].tolist() == [0, 1, 2, 3, 4, 0, 1, 2] and run.first[:5].tolist() == [0, 1, 2, 3, 4]
    # the same on the packed route: (Int32, Int16)
    b16 = numbers(np.array([10, 10, 11, 0, 3, 10, 10, 11], np.int16), valid=[1, 1, 1, 0, 0, 1, 1, 1])
    run = both(ctx, [a, b16])
    assert run.ids[:8].tolist() == [0, 1, 2, 3, 4, 0, 1, 2]
    # one row; no rows: nothing written, count 0
    for cols in ([numbers(np.array([3], np.int32)), strings([b"x"])], [numbers(np.array([3], np.int32), valid=[0]), strings([None])],
                 [numbers(np.array([3], np.int32), valid=[0]), numbers(np.array([3], np.int8))]):
        assert both(ctx, cols).ngroups == 1
    for cols in ([numbers(np.zeros(0, np.int32)), strings([])], [numbers(np.zeros(0, np.int32)), numbers(np.zeros(0, np.int8))],
                 [strings([])], [numbers(np.zeros(0, np.uint64))]):
        run = both(ctx, cols)
        assert run.ngroups == 0 and run.ids[0] == A5_32 and run.first[0] == A5_64


@pytest.mark.gpu
def test_the_payload_under_a_null_is_not_looked_at(ctx):
    valid = [0, 0, 1, 1, 0]
    a = np.array([7, 9, 7, 9, 1234567], np.int32)              # rows 0, 1, 4: null, with different bytes under the null
    for other in (numbers(np.array([2, 2, 2, 2, 2], np.int8)), strings([b"s"] * 5)):          # the packed route, the tuple route
        run = both(ctx, [numbers(a, valid), other])
        assert run.ids[:5].tolist() == [0, 0, 1, 2, 0]
    # a var-length column: different bytes, and different lengths, under its nulls
    s = Col("str", [b"xx", b"yyy", b"xx", b"", b"z"], [0, 0, 1, 1, 0])
    run = both(ctx, [s, numbers(np.array([1, 1, 1, 1, 1], np.int64))])
    assert run.ids[:5].tolist() == [0, 0, 1, 2, 0]
    # a Boolean column
    run = both(ctx, [bools([1, 0, 1, 0], valid=[0, 0, 1, 1]), numbers(np.array([4, 4, 4, 4], np.int8))])
    assert run.ids[:4].tolist() == [0, 0, 1, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("large", [False, True])
def test_columns_are_not_concatenated(ctx, large):
    a = [b"ab", b"a", b"abc", b"ab", b"", b"abc", b"abc", None, b""]
    b = [b"c", b"bc", b"", b"c", b"abc", None, b"", b"abc", None]
    run = both(ctx, [strings(a, large), strings(b, large)])
    assert run.ids[:9].tolist() == [0, 1, 2, 0, 3, 4, 2, 5, 6]             # "" is not null, ("abc", "") is not ("", "abc")
    run = both(ctx, [strings(a, large), strings(b, not large)])
    assert run.ngroups == 7


def random_valid(rng, n, p=0.85):
    return rng.random(n) < p


@pytest.mark.gpu
def test_layouts(ctx):
    rng = np.random.default_rng(3)
    n = 1500
    tag = numbers(drawn(rng, np.arange(3, dtype=np.int8), n))
    fsb3 = rng.integers(0, 256, (40, 3), dtype=np.uint8)
    dec128 = rng.integers(0, 256, (40, 16), dtype=np.uint8)
    dec128[:20, 1:] = dec128[0, 1:]                              # values that differ in their first byte only
    five = rng.integers(0, 256, (40, 5), dtype=np.uint8)
    for pool in (fsb3, dec128, five):
        rows = drawn(rng, pool, n)
        both(ctx, [slots(rows, random_valid(rng, n))])                               # alone: the fixed-width encoder
        both(ctx, [slots(rows, random_valid(rng, n)), tag])
        both(ctx, [tag, slots(rows)])
    # a Boolean column at every bit offset, alone and on both tuple routes
    for off in range(8):
        bits = rng.random(n) < 0.5
        assert both(ctx, [bools(bits, off=off)]).ngroups == 2
        assert both(ctx, [bools(bits, random_valid(rng, n), off=off)]).ngroups == 3
        both(ctx, [bools(bits, random_valid(rng, n), off=off), tag])
        both(ctx, [strings(drawn(rng, [b"p", b"q", b""], n)), bools(bits, random_valid(rng, n), off=off)])
    # (Boolean, Int16, String, Decimal256)
    dec256 = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    dec256[1:, :31] = dec256[0, :31]                             # … that differ in their last byte only
    cols = [bools(rng.random(n) < 0.5, random_valid(rng, n)), numbers(drawn(rng, np.array([-1, 0, 300], np.int16), n), random_valid(rng, n)),
            strings(drawn(rng, [b"", b"a", b"ab", None, b"a much longer string than eight bytes"], n)), slots(drawn(rng, dec256, n), random_valid(rng, n))]
    assert both(ctx, cols).ngroups > 100


@pytest.mark.gpu
def test_both_sides_of_the_64_bit_budget(ctx):
    """value bits + one bit per column with a validity buffer: (4, 4) without validity is 64 bits (packed, and the all-ones word occurs),
    (4, 4) with one nullable column is 65 (hashed where it lies); (4, 2, 1) all nullable is 59; eight 1-byte columns are 64 and 65"""
    rng = np.random.default_rng(4)
    n = 4000
    pool32 = np.array([0xFFFFFFFF, 0, 1, 0x80000000, 0xFFFFFFFE], np.uint32)
    a, b = drawn(rng, pool32, n), drawn(rng, pool32, n)
    a[5] = b[5] = a[77] = b[77] = 0xFFFFFFFF                     # the tables' EMPTY marker as a key, not in the first row
    assert both(ctx, [numbers(a), numbers(b)]).ngroups == 25
    assert both(ctx, [numbers(a), numbers(b, random_valid(rng, n))]).ngroups == 30
    c16, c8 = drawn(rng, np.array([0xFFFF, 0, 7], np.uint16), n), drawn(rng, np.array([0xFF, 0], np.uint8), n)
    both(ctx, [numbers(a, random_valid(rng, n)), numbers(c16, random_valid(rng, n)), numbers(c8, random_valid(rng, n))])
    pool8 = np.array([0xFF, 0, 0x80], np.uint8)
    eight = [drawn(rng, pool8, n) for _ in range(8)]
    for col in eight:
        col[9] = col[300] = 0xFF
    both(ctx, [numbers(col) for col in eight])
    both(ctx, [numbers(col, random_valid(rng, n) if j == 3 else None) for j, col in enumerate(eight)])


@pytest.mark.gpu
def test_row_counts_around_a_workgroup_step(ctx):
    block = source_constant("ah_hashing.h", "kBlock")
    steps = {block * source_constant("ah_group_keys.hip", "kPackRows"), block * source_constant("ah_hash.hip", "kInsertRows")}
    sizes = sorted({s + d for s in steps for d in (-1, 0, 1)} | {3 * s + 1 for s in steps})
    assert 1024 in sizes
    for n in sizes:
        rng = np.random.default_rng(n)
        a = drawn(rng, np.arange(-20, 20, dtype=np.int32), n)
        a[n - 1] = 1000                                          # the last row is a group of its own
        v = random_valid(rng, n)
        v[n - 1] = True
        run = both(ctx, [numbers(a, v), numbers(drawn(rng, np.arange(5, dtype=np.int16), n))])
        assert int(run.first[run.ngroups - 1]) == n - 1
        run = both(ctx, [numbers(a, v), strings(drawn(rng, [b"", b"x", b"xy", None], n))])
        assert int(run.first[run.ngroups - 1]) == n - 1


@pytest.mark.gpu
def test_slices(ctx):
    n = 2500
    for k in range(8):
        rng = np.random.default_rng(70 + k)
        o = [(k + 3 * j) % 8 for j in range(4)]
        narrow = [numbers(drawn(rng, np.arange(9, dtype=np.int32), n), random_valid(rng, n), o[0]), bools(rng.random(n) < 0.5, random_valid(rng, n), o[1]),
                  numbers(drawn(rng, np.arange(4, dtype=np.int16), n), None, o[2])]
        both(ctx, narrow, seed=k)
        wide = [strings(drawn(rng, [b"a", b"bb", b"", None, b"a string of more than eight bytes"], n), off=o[0]),
                slots(drawn(rng, rng.integers(0, 256, (6, 3), dtype=np.uint8), n), random_valid(rng, n), o[1]),
                bools(rng.random(n) < 0.5, random_valid(rng, n), o[2]), strings(drawn(rng, [b"x", b"y", None], n), large=True, off=o[3])]
        both(ctx, wide, seed=k)


@pytest.mark.gpu
def test_routes_of_the_packed_column(ctx):
    """2^17 rows of (Int32, Int32), about 2^15 distinct tuples: the encoder's default route, and the partition-first routes forced"""
    n = 1 << 17
    rng = np.random.default_rng(8)
    a, b = rng.integers(0, 256, n).astype(np.int32) - 128, rng.integers(0, 128, n).astype(np.int32) * 1000003
    runs = []
    try:
        for option in (None, 8, 11):
            if option is not None:
                ctx.set_option("encode_partition", option)
            runs.append(Run(ctx, [numbers(a), numbers(b)], n))
    finally:
        ctx.set_option("encode_partition", 1)
    check(runs[0], [numbers(a), numbers(b)])
    assert 30000 < runs[0].ngroups <= 1 << 15
    for r in runs[1:]:
        assert r.ngroups == runs[0].ngroups and r.ids.tobytes() == runs[0].ids.tobytes() and r.first.tobytes() == runs[0].first.tobytes()


@pytest.mark.gpu
def test_cardinality_extremes_on_the_tuple_route(ctx):
    n = 1 << 17
    rng = np.random.default_rng(9)
    # all distinct: the table grows (or overflows and is retried)
    s = [b"key-%d" % (i * 7919 % n) for i in range(n)]
    run = both(ctx, [strings(s), numbers(np.arange(n, dtype=np.int64) // 2)])
    assert run.ngroups == n
    # one tuple owns 90 % of the rows, first seen at row 0
    hot = rng.random(n) < 0.9
    hot[0] = True
    s = [b"hot" if h else b"cold-%d" % j for h, j in zip(hot.tolist(), rng.integers(0, 500, n).tolist())]
    v = np.where(hot, 42, rng.integers(0, 3, n)).astype(np.int64)
    run = both(ctx, [strings(s), numbers(v)])
    assert int(run.ids[0]) == 0 and int((run.ids[:n] == 0).sum()) == int(hot.sum())


def encoder_outputs(ctx, n, call):
    """ids and first rows of one of the encoders with encode_nulls = 1: call(out_ids, out_first_rows) -> ndict"""
    ids_buf, first_buf = ctx.alloc((n + 1) * 4 + 64), ctx.alloc((n + 2) * 8 + 64)
    ids_buf.memset(0xA5)
    first_buf.memset(0xA5)
    nd = call(ids_buf, first_buf)
    ctx.sync()
    out = nd, ids_buf.download(np.uint32, n + 1), first_buf.download(np.uint64, nd + 1)
    ids_buf.free()
    first_buf.free()
    return out


@pytest.mark.gpu
def test_a_single_key_is_the_matching_encoder(ctx):
    rng = np.random.default_rng(10)
    n, off = 30001, 5
    # uint64: null keys and the all-ones key
    k = (rng.integers(0, 900, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15))
    k[k == k[3]] = np.uint64(0xFFFFFFFFFFFFFFFF)
    kv = random_valid(rng, n, 0.95)
    col = numbers(k, kv, off)
    run = both(ctx, [col])
    kb, vb = ctx.to_device(k, 64), ctx.to_device(col._bits(rng, kv), 64)
    nd, ids, _ = encoder_outputs(ctx, n, lambda i, f: ctx.hash_u64_encode(kb, vb, off, n, True, i, None, None)[0])
    assert nd == run.ngroups and ids[:n].tobytes() == run.ids[:n].tobytes()
    # (ah_hash_u64_encode has no first rows: those of the group-by over the same keys)
    outs = [ctx.alloc((n + 2) * 8 + 64) for _ in range(4)]
    ng, _ = ctx.hash_sum("i64", kb, vb, off, kb, None, 0, n, outs[0], outs[1], outs[2], outs[3])
    ctx.sync()
    assert ng == run.ngroups and outs[3].download(np.uint64, ng).tobytes() == run.first[:ng].tobytes()
    for b in [kb, vb] + outs:
        b.free()
    # String
    s = strings(drawn(rng, [b"", b"a", b"ab", None, b"longer than eight bytes", b"longer than eight bytez"], n), off=off)
    run = both(ctx, [s])
    d = s.upload(ctx, np.random.default_rng(1))
    nd, ids, first = encoder_outputs(ctx, n, lambda i, f: ctx.hash_binary_encode(4, d[3], d[4], d[5], off, n, True, i, None, f)[0])
    s.free()
    assert nd == run.ngroups == 6 and ids.tobytes() == run.ids.tobytes() and first.tobytes() == run.first.tobytes()
    # FixedSizeBinary[3]
    f3 = slots(drawn(rng, rng.integers(0, 256, (50, 3), dtype=np.uint8), n), random_valid(rng, n), off)
    run = both(ctx, [f3])
    d = f3.upload(ctx, np.random.default_rng(1))
    nd, ids, first = encoder_outputs(ctx, n, lambda i, f: ctx.hash_fixed_encode(3, d[4], d[5], off, n, True, i, None, f, None)[0])
    f3.free()
    assert nd == run.ngroups and ids.tobytes() == run.ids.tobytes() and first.tobytes() == run.first.tobytes()


DTYPES = {"i64": np.int64, "u64": np.uint64, "f64": np.float64}


def sliced_bitmap(rng, valid_rows, off):
    n = len(valid_rows)
    bits = rng.random(off + n + 13) < 0.5
    bits[off:off + n] = valid_rows
    return pack(bits)


@pytest.mark.gpu
@pytest.mark.parametrize("card", [700, 9000])
def test_aggregates_over_ids_are_the_existing_group_by(ctx, card):
    """ids from ah_group_ids over one uint64 key column, then ah_group_sum_* / ah_group_min_max_*: the bytes of ah_hash_sum_* /
    ah_hash_min_max_* on the same rows — on both sides of the 4096-group LDS table, value validity sliced"""
    n, koff, voff = 50001, 3, 6
    rng = np.random.default_rng(card)
    k = np.concatenate([rng.permutation(card), rng.integers(0, card, n - card)]).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    k[k == k[0]] = np.uint64(0xFFFFFFFFFFFFFFFF)
    kv = rng.random(n) < 0.97
    kv[:card] = True                                             # (the rows that introduce the keys: a null there could take a key away)
    kcol = numbers(k, kv, koff)
    run = Run(ctx, [kcol], n, keep=True)
    check(run, [kcol])
    ng = run.ngroups
    assert ng == card + 1
    kb, kvb = ctx.to_device(k, 64), ctx.to_device(sliced_bitmap(rng, kv, koff), 64)
    vvb = ctx.to_device(sliced_bitmap(rng, rng.random(n) < 0.9, voff), 64)
    ints = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64)
    whole = rng.integers(-10**6, 10**6, n).astype(np.float64)                           # exact in any order
    mixed = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)
    mixed[rng.random(n) < 0.02] = np.nan
    room = (n + 2) * 8 + 64

    def outputs(count):
        bufs = [ctx.alloc(room) for _ in range(count)]
        for b in bufs:
            b.memset(0xA5)
        return bufs

    def same(name, a, b):
        x, y = a.download(np.uint64, ng + 1), b.download(np.uint64, ng + 1)
        bad = np.flatnonzero(x[:ng] != y[:ng])
        assert bad.size == 0, f"{name}: group {bad[0]} of {ng}: {int(x[bad[0]]):#018x} over ids, {int(y[bad[0]]):#018x} from the group-by"
        assert x[ng] == A5_64, f"{name}: wrote past the last group"

    for kind, vals in (("i64", ints), ("f64", whole), ("f64", mixed)):
        vb = ctx.to_device(vals, 64)
        keys_o, sums_o, counts_o, first_o, sums, counts = outputs(6)
        assert ctx.hash_sum(kind, kb, kvb, koff, vb, vvb, voff, n, keys_o, sums_o, counts_o, first_o)[0] == ng
        ctx.group_sum(kind, run.ids_buf, ng, vb, vvb, voff, n, sums, counts)
        ctx.sync()
        same(kind + " sums", sums, sums_o)
        same(kind + " counts", counts, counts_o)
        assert first_o.download(np.uint64, ng).tobytes() == run.first[:ng].tobytes()
        for b in (vb, keys_o, sums_o, counts_o, first_o, sums, counts):
            b.free()
    for kind, vals in (("i64", ints), ("u64", ints.view(np.uint64)), ("f64", mixed)):
        vb = ctx.to_device(vals, 64)
        keys_o, mins_o, maxs_o, counts_o, mins, maxs, counts = outputs(7)
        assert ctx.hash_min_max(kind, kb, kvb, koff, vb, vvb, voff, n, keys_o, mins_o, maxs_o, counts_o)[0] == ng
        ctx.group_min_max(kind, run.ids_buf, ng, vb, vvb, voff, n, mins, maxs, counts)
        ctx.sync()
        same(kind + " mins", mins, mins_o)
        same(kind + " maxs", maxs, maxs_o)
        same(kind + " counts", counts, counts_o)
        for b in (vb, keys_o, mins_o, maxs_o, counts_o, mins, maxs, counts):
            b.free()
    for b in (kb, kvb, vvb):
        b.free()
    run.free()


@pytest.mark.gpu
def test_end_to_end_against_the_restatement_and_pyarrow(ctx):
    """(String, Int32) keys -> ids -> sum and min / max -> the key columns gathered at the groups' first rows with Take"""
    import pyarrow as pa
    n = 20000
    rng = np.random.default_rng(12)
    names = drawn(rng, [b"north", b"south", b"", None, b"a region with a long name", b"east"], n)
    days = rng.integers(0, 40, n).astype(np.int32)
    dvalid = random_valid(rng, n, 0.9)
    vals = rng.integers(-10**9, 10**9, n).astype(np.int64)
    vvalid = random_valid(rng, n, 0.8)
    scol, dcol = strings(names), numbers(days, dvalid)
    run = Run(ctx, [scol, dcol], n, keep=True)
    want_ids, want_first = check(run, [scol, dcol])
    ng = run.ngroups
    vb, vvb = ctx.to_device(vals, 64), ctx.to_device(pack(vvalid), 64)
    sums, counts, mins, maxs, counts2 = [ctx.alloc((ng + 1) * 8 + 64) for _ in range(5)]
    ctx.group_sum("i64", run.ids_buf, ng, vb, vvb, 0, n, sums, counts)
    ctx.group_min_max("i64", run.ids_buf, ng, vb, vvb, 0, n, mins, maxs, counts2)
    ctx.sync()
    got = {name: b.download(np.int64, ng).tolist() for name, b in (("sum", sums), ("count", counts), ("min", mins), ("max", maxs), ("count2", counts2))}
    # the restatement of the aggregates, by id
    exp = {name: [0] * ng for name in ("sum", "count", "min", "max")}
    for g, x, ok in zip(want_ids, vals.tolist(), vvalid.tolist()):
        if ok:
            exp["min"][g] = x if exp["count"][g] == 0 else min(exp["min"][g], x)
            exp["max"][g] = x if exp["count"][g] == 0 else max(exp["max"][g], x)
            exp["sum"][g] += x
            exp["count"][g] += 1
    for name in ("sum", "count", "min", "max"):
        assert got[name] == exp[name], name
    assert got["count2"] == exp["count"]
    # the groups' keys: Take of each key column at first_rows (int64 indices)
    sd, dd = scol.upload(ctx, rng), dcol.upload(ctx, rng)
    out_days, out_dvalid = ctx.alloc(ng * 4 + 64), ctx.alloc(ng // 8 + 64)
    ctx.take_primitive(4, dd[4], dd[5], 0, n, 8, True, run.first_buf, None, 0, ng, True, out_days, out_dvalid)
    out_offsets, out_svalid = ctx.alloc((ng + 1) * 4 + 64), ctx.alloc(ng // 8 + 64)
    _, total = ctx.take_binary_offsets(4, sd[3], sd[5], 0, n, 8, True, run.first_buf, None, 0, ng, out_offsets, out_svalid)
    out_data = ctx.alloc(total + 64)
    ctx.take_binary_data(4, sd[3], sd[4], 0, 8, run.first_buf, ng, out_offsets, out_data)
    ctx.sync()
    gd, gdv = out_days.download(np.int32, ng), np.unpackbits(out_dvalid.download(np.uint8, ng // 8 + 1), bitorder="little")[:ng].astype(bool)
    go, gs = out_offsets.download(np.int32, ng + 1), out_data.download(np.uint8, total).tobytes()
    gsv = np.unpackbits(out_svalid.download(np.uint8, ng // 8 + 1), bitorder="little")[:ng].astype(bool)
    group_keys = [((gs[go[g]:go[g + 1]] if gsv[g] else None), (int(gd[g]) if gdv[g] else None)) for g in range(ng)]
    assert group_keys == [(names[r], (int(days[r]) if dvalid[r] else None)) for r in want_first]
    assert len(set(group_keys)) == ng
    # the third opinion, matched by key tuple
    t = pa.table({"s": pa.array(names, pa.binary()), "d": pa.array(days, mask=~dvalid), "v": pa.array(vals, mask=~vvalid)})
    r = t.group_by(["s", "d"], use_threads=False).aggregate([("v", "sum"), ("v", "min"), ("v", "max"), ("v", "count")])
    theirs = {(s, d): row for s, d, *row in zip(*(r[c].to_pylist() for c in ("s", "d", "v_sum", "v_min", "v_max", "v_count")))}
    assert len(theirs) == ng
    for g, key in enumerate(group_keys):
        tsum, tmin, tmax, tcount = theirs[key]
        assert tcount == got["count"][g], key
        if tcount:
            assert (tsum, tmin, tmax) == (got["sum"][g], got["min"][g], got["max"][g]), key
        else:
            assert tsum is None and tmin is None and got["sum"][g] == got["min"][g] == got["max"][g] == 0
    scol.free()
    dcol.free()
    for b in (vb, vvb, sums, counts, mins, maxs, counts2, out_days, out_dvalid, out_offsets, out_svalid, out_data):
        b.free()
    run.free()


@pytest.mark.gpu
def test_two_calls_give_the_same_bytes(ctx):
    n = 1 << 16
    rng = np.random.default_rng(13)
    a, b = rng.integers(0, 300, n).astype(np.int32), rng.integers(0, 60, n).astype(np.int16)
    s = drawn(rng, [b"k%d" % j for j in range(200)] + [None], n)
    v = random_valid(rng, n)
    for make in (lambda: [numbers(a, v), numbers(b)], lambda: [strings(s), numbers(a, v)]):
        one, two = Run(ctx, make(), n, seed=1), Run(ctx, make(), n, seed=2)           # (other junk around the slices)
        assert one.ngroups == two.ngroups and one.ids.tobytes() == two.ids.tobytes() and one.first.tobytes() == two.first.tobytes()
        check(one, make())


@pytest.mark.gpu
def test_argument_checks(ctx):
    from arrow_go_amd import _native as N
    bufs = [ctx.alloc(4096) for _ in range(6)]
    d, o, ids, first, x, y = bufs
    fixed = (0, 4, 0, None, d, None, 0)
    with pytest.raises(N.ErrInvalid, match="group_ids: 1 to 8 key columns"):
        ctx.group_ids([], 4, ids, first)
    with pytest.raises(N.ErrInvalid, match="group_ids: 1 to 8 key columns"):
        ctx.group_ids([fixed] * 9, 4, ids, first)
    with pytest.raises(N.ErrInvalid, match="group_ids: negative length/offset"):
        ctx.group_ids([fixed], -1, ids, first)
    with pytest.raises(N.ErrInvalid, match="group_ids: negative length/offset"):
        ctx.group_ids([fixed, (0, 4, 0, None, d, None, -2)], 4, ids, first)
    with pytest.raises(N.ErrInvalid, match="group_ids: null buffer"):
        ctx.group_ids([fixed, (0, 2, 0, None, None, None, 0)], 4, ids, first)
    with pytest.raises(N.ErrInvalid, match="group_ids: null buffer"):
        ctx.group_ids([(4, 0, 0, None, d, None, 0)], 4, ids, first)
    with pytest.raises(N.ErrInvalid, match="group_ids: null buffer"):
        ctx.group_ids([fixed], 4, ids, None)
    with pytest.raises(N.ErrInvalid, match="group_ids: offset width must be 0, 4 or 8"):
        ctx.group_ids([(3, 0, 0, o, d, None, 0)], 4, ids, first)
    with pytest.raises(N.ErrInvalid, match="group_ids: a bits column has no byte width or offsets"):
        ctx.group_ids([(0, 1, 1, None, d, None, 0)], 4, ids, first)
    with pytest.raises(N.ErrInvalid, match="group_ids: fixed width must be 1..4096 bytes"):
        ctx.group_ids([(0, 0, 0, None, d, None, 0)], 4, ids, first)
    with pytest.raises(N.ErrInvalid, match="group_ids: fixed width must be 1..4096 bytes"):
        ctx.group_ids([(0, 4097, 0, None, d, None, 0)], 4, ids, first)
    for kind in ("i64", "f64"):
        with pytest.raises(N.ErrInvalid, match="group_sum: negative length/offset"):
            ctx.group_sum(kind, ids, -1, d, None, 0, 4, x, y)
        with pytest.raises(N.ErrInvalid, match="group_sum: negative length/offset"):
            ctx.group_sum(kind, ids, 2, d, None, -1, 4, x, y)
        with pytest.raises(N.ErrInvalid, match="group_sum: negative length/offset"):
            ctx.group_sum(kind, ids, 2, d, None, 0, -4, x, y)
        with pytest.raises(N.ErrInvalid, match="group_sum: null buffer"):
            ctx.group_sum(kind, ids, 2, None, None, 0, 4, x, y)
    for kind in ("i64", "u64", "f64"):
        with pytest.raises(N.ErrInvalid, match="group_min_max: negative length/offset"):
            ctx.group_min_max(kind, ids, -1, d, None, 0, 4, x, y, first)
        with pytest.raises(N.ErrInvalid, match="group_min_max: null buffer"):
            ctx.group_min_max(kind, ids, 2, d, None, 0, 4, x, None, first)
    with pytest.raises(ValueError):
        ctx.group_sum("u32", ids, 2, d, None, 0, 4, x, y)
    with pytest.raises(ValueError):
        ctx.group_min_max("f32", ids, 2, d, None, 0, 4, x, y, first)
    # no groups: nothing touched
    x.memset(0xA5)
    ctx.group_sum("i64", None, 0, None, None, 0, 0, x, y)
    ctx.sync()
    assert x.download(np.uint8, 64).tolist() == [0xA5] * 64
    for b in bufs:
        b.free()
