"""GPU parity tests proper: the HIP path through the C ABI vs the CPU oracle on the same
seeded inputs (sizes the oracle finishes in seconds), bit-exact for every integer /
byte / bitmap / index result; Float64 Sum within 1 ULP of the exact sum (tolerance
stated at the assertion).  Edge cases follow the reference's tests: empty and ragged
lengths, non-zero bit offsets (sliced arrays), misaligned value pointers, nulls in
either input, tile/wave boundaries of our own kernels.
"""
import math

import numpy as np
import pytest

from tests import oracle_lib as OL
from tests.backends import OracleBackend, HipBackend, STATUS_OK, STATUS_EINVALID, STATUS_EINDEX, STATUS_EOVERFLOW
from tests.test_sum_nonfinite import seq_sum

pytestmark = pytest.mark.gpu

ADD, SUB, MUL = 0, 1, 2
EQ, NE, GT, GE = 0, 1, 2, 3
AA, AS, SA = 0, 1, 2
DROP, EMIT = 0, 1

# lengths around our kernels' boundaries: vector (2..16 elems), wave (64), block
# iteration (256*4 vectors), filter tile (2048..16384 rows), plus ragged primes
SIZES = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 257, 1023, 1025, 2047, 2048, 2049, 4099, 16384, 16385, 70001, 300007]


@pytest.fixture(scope="module")
def hip(ctx):
    return HipBackend(ctx, dirty_outputs=True)


@pytest.fixture(scope="module")
def orc_be():
    return OracleBackend()


def rand(rng, dtype, n, small=False):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        a = (rng.standard_normal(n) * 1e3).astype(dt)
        if n > 8 and not small:
            a[rng.integers(0, n, 4)] = [np.nan, np.inf, -np.inf, -0.0]
        return a
    if small:
        return rng.integers(0, 5, n).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def same_bits_or_both_nan(got, exp):
    """Bit-exact, except that a NaN result may carry a different payload / sign: x86 SSE
    returns the negative "real indefinite" qNaN (0xFFF8…) for inf−inf and propagates the
    first operand's payload, CDNA4 returns the positive canonical qNaN (0x7FF8…).  IEEE-754
    leaves both unspecified and the reference's own tests compare with array.ApproxEqual
    (NaN == NaN), so this is the one place float add/sub/mul is not byte-compared."""
    if got.tobytes() == exp.tobytes():
        return True
    if got.dtype.kind != "f":
        return False
    gb, eb = got.view(f"u{got.dtype.itemsize}"), exp.view(f"u{exp.dtype.itemsize}")
    diff = gb != eb
    return bool((np.isnan(got[diff]) & np.isnan(exp[diff])).all())


def rand_bits(rng, nbits, p=0.5):
    return OL.pack_bits(rng.random(nbits) < p) if nbits else np.zeros(1, np.uint8)


# ---- Sum ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES + [1 << 20])
@pytest.mark.parametrize("misalign", [0, 1])
def test_sum_int_bit_exact(hip, orc_be, n, misalign):
    rng = np.random.default_rng(n + misalign)
    for dt in (np.int64, np.uint64):
        a = rand(rng, dt, n)
        assert hip.sum(a, misalign) == orc_be.sum(a)


@pytest.mark.parametrize("n", SIZES + [1 << 20])
@pytest.mark.parametrize("misalign", [0, 1])
def test_sum_float64(hip, orc_be, n, misalign):
    rng = np.random.default_rng(n * 3 + misalign)
    # (a) integer-valued data < 2^53: exact in any order → bit-exact (the reference's only pinned case)
    a = rng.integers(-1000, 1000, n).astype(np.float64)
    assert hip.sum(a, misalign) == float(a.astype(np.int64).sum())
    # (b) general data: |gpu − exact| ≤ 1 ULP(exact), exact = correctly rounded sum (math.fsum)
    b = rng.uniform(-1, 1, n)
    exact = math.fsum(b.tolist())
    got = hip.sum(b, misalign)
    if n <= 31:   # up to 31 rows: the reference's own sequential loop, bit for bit (tests/test_sum_short.py)
        assert got == seq_sum(b), (got, seq_sum(b))
    else:
        assert abs(got - exact) <= math.ulp(exact) if exact != 0 else abs(got) <= 5e-324 * 4, (got, exact)
    # (c) heavy cancellation (condition number ≈ 1e9), where both reference orders lose ~9
    # digits.  Double-double bound: |got − exact| ≤ ulp(exact) + n·2^-104·Σ|x|
    c = np.concatenate([b * 1e8, -b * 1e8, rng.uniform(-1, 1, max(n // 3, 1))])
    rng.shuffle(c)
    exact = math.fsum(c.tolist())
    got = hip.sum(c, misalign)
    bound = max(math.ulp(exact), 5e-324) + len(c) * 2.0**-104 * float(np.abs(c).sum())
    if len(c) <= 31:   # the sequential loop loses the digits the reference loses
        assert got == seq_sum(c), (got, seq_sum(c))
    else:
        assert abs(got - exact) <= bound, (got, exact, bound)


def test_sum_float64_vs_reference_orders(hip):
    """The GPU result must sit inside the gap between the reference's own two paths
    (AVX2 order vs noasm order) — both are approximations of the same exact sum."""
    o = OL.load_oracle()
    rng = np.random.default_rng(11)
    a = rng.uniform(-1, 1, 1 << 20)
    seq, avx = float(o.sum_float64_seq(a)), float(o.sum_float64_avx2order(a))
    got, exact = hip.sum(a), math.fsum(a.tolist())
    assert abs(got - exact) <= math.ulp(exact)
    assert abs(got - exact) <= max(abs(seq - exact), abs(avx - exact)) + math.ulp(exact)


# ---- arithmetic ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", OL.ALL_DTYPES, ids=str)
@pytest.mark.parametrize("op", [ADD, SUB, MUL])
def test_arithmetic_bit_exact(hip, orc_be, dtype, op):
    rng = np.random.default_rng(op * 31 + OL.TYPE_IDS[np.dtype(dtype)])
    for n in [0, 1, 17, 1025, 4099, 70001]:
        l, r, s = rand(rng, dtype, n), rand(rng, dtype, n), rand(rng, dtype, 1)
        for shape, a, b in [(AA, l, r), (AS, l, s), (SA, s, r)]:
            for mis in (0, 1):
                got, exp = hip.arithmetic(op, shape, a, b, mis), orc_be.arithmetic(op, shape, a, b)
                assert same_bits_or_both_nan(got, exp), (dtype, op, shape, n, mis)


@pytest.mark.parametrize("dtype", OL.ALL_DTYPES, ids=str)
def test_unary_bit_exact(hip, orc_be, dtype):
    rng = np.random.default_rng(5)
    for n in [1, 17, 4099]:
        a = rand(rng, dtype, n)
        for op in (4, 5, 20):
            for mis in (0, 1):
                assert hip.arithmetic_unary(op, a, mis).tobytes() == orc_be.arithmetic_unary(op, a).tobytes(), (dtype, op, n)


@pytest.mark.parametrize("dtype", OL.INT_DTYPES, ids=str)
def test_checked_bit_exact(hip, orc_be, dtype):
    rng = np.random.default_rng(9)
    info = np.iinfo(dtype)
    for n in [1, 65, 3001]:
        for op in (21, 22, 23):
            # (i) small operands: no overflow → outputs must match including zeros under nulls
            l = rng.integers(6, 11, n).astype(dtype); r = rng.integers(0, 6, n).astype(dtype)  # l > r (unsigned SUB in range), l*r <= 50 (int8 MUL in range)
            lv, rv = rand_bits(rng, n + 5, 0.8), rand_bits(rng, n + 9, 0.8)
            st_h, out_h = hip.arithmetic_checked(op, AA, l, lv, 5, r, rv, 9)
            st_o, out_o = orc_be.arithmetic_checked(op, AA, l, lv, 5, r, rv, 9)
            assert st_h == st_o == STATUS_OK and out_h.tobytes() == out_o.tobytes()
            # (ii) full-range operands: the error decision must match the reference's carry test
            l, r = rand(rng, dtype, n), rand(rng, dtype, n)
            st_h, _ = hip.arithmetic_checked(op, AA, l, lv, 5, r, rv, 9)
            st_o, _ = orc_be.arithmetic_checked(op, AA, l, lv, 5, r, rv, 9)
            assert st_h == st_o, (dtype, op, n)


@pytest.mark.parametrize("dtype", OL.INT_DTYPES, ids=str)
def test_checked_all_shapes_bit_exact(hip, orc_be, dtype):
    """The three checked ops through the one validity-aware kernel, in every shape.  Lengths (V = 16 / width elements per vector): an empty
    call, a tail-only call, one vector short of / exactly / just past one vector, one full workgroup plus a ragged tail, a second
    workgroup; value pointers 16-byte aligned and one element off; validity at bit offsets 5 and 9, 80 % valid; a valid and a null scalar."""
    rng = np.random.default_rng(10)
    V = 16 // np.dtype(dtype).itemsize
    for n in [0, 1, V - 1, V, V + 1, 256 * V + V - 1, 512 * V + 1]:
        lv, rv = rand_bits(rng, n + 5, 0.8), rand_bits(rng, n + 9, 0.8)
        for small in (True, False):
            if small:  # nothing overflows (l > r: unsigned SUB in range, l * r <= 50: int8 MUL in range) → output bytes, zeros under nulls
                l, r = rng.integers(6, 11, n).astype(dtype), rng.integers(0, 6, n).astype(dtype)
                ls, rs = np.array([8], dtype), np.array([3], dtype)
            else:      # full range: the error decision must be the reference's carry test
                l, r, ls, rs = rand(rng, dtype, n), rand(rng, dtype, n), rand(rng, dtype, 1), rand(rng, dtype, 1)
            cases = [(AA, (l, lv, 5, r, rv, 9), True)]
            cases += [(AS, (l, lv, 5, rs, None, 0), sv) for sv in (True, False)] + [(SA, (ls, None, 0, r, rv, 9), sv) for sv in (True, False)]
            for op in (21, 22, 23):
                for shape, args, sv in cases:
                    st_o, out_o = orc_be.arithmetic_checked(op, shape, *args, scalar_valid=sv)
                    for mis in (0, 1):
                        st_h, out_h = hip.arithmetic_checked(op, shape, *args, scalar_valid=sv, misalign=mis)
                        assert st_h == st_o, (dtype, op, shape, n, sv, mis, small)
                        if small:
                            assert st_o == STATUS_OK and out_h.tobytes() == out_o.tobytes(), (dtype, op, shape, n, sv, mis)
    # Mul tests EVERY slot (ScalarBinary): the only overflowing product under a null — in a vector's body, then in the tail
    n = 4 * V + 1
    info = np.iinfo(dtype)
    for k in (1, n - 1):
        l, r = rng.integers(6, 11, n).astype(dtype), rng.integers(0, 6, n).astype(dtype)
        l[k], r[k] = info.max, 2
        valid = np.ones(n + 5, bool)
        valid[5 + k] = False
        lv = OL.pack_bits(valid)
        for op, want in ((23, STATUS_EOVERFLOW), (21, STATUS_OK)):   # … which Add, a NotNull op, does not see
            st_o, _ = orc_be.arithmetic_checked(op, AA, l, lv, 5, r, None, 0)
            st_h, _ = hip.arithmetic_checked(op, AA, l, lv, 5, r, None, 0)
            assert st_o == want and st_h == st_o, (dtype, op, k)


# ---- compare ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", OL.ALL_DTYPES, ids=str)
def test_compare_bit_exact(hip, orc_be, dtype):
    rng = np.random.default_rng(21)
    dt = np.dtype(dtype)
    for n in [1, 5, 31, 33, 64, 257, 1025, 8191, 70001]:
        l, r = rand(rng, dtype, n, small=True), rand(rng, dtype, n, small=True)
        if dt.kind == "f" and n > 4:
            l[1] = np.nan; r[2] = np.nan
        s = np.array([2], dtype=dt)
        for cmpop in (EQ, NE, GT, GE):
            for shape, a, b in [(AA, l, r), (AS, l, s), (SA, s, r)]:
                for offset, fill in [(0, 0x00), (3, 0xFF), (7, 0x00)]:
                    init = np.full((offset + n + 7) // 8 + 2, fill, np.uint8)
                    got = hip.comparison(cmpop, shape, a, b, init, offset, misalign=offset & 1)
                    exp = orc_be.comparison(cmpop, shape, a, b, init, offset)
                    assert got.tobytes() == exp.tobytes(), (dtype, cmpop, shape, n, offset)


# ---- bitmaps ------------------------------------------------------------------------------
def test_bitmap_ops_random(hip, orc_be):
    rng = np.random.default_rng(33)
    for n in [1, 7, 64, 65, 1000, 4097, 100003]:
        for lo, ro, oo in [(0, 0, 0), (1, 5, 3), (64, 8, 16), (13, 21, 38), (7, 0, 63), (120, 75, 65536 % 977)]:
            l, r = rand_bits(rng, lo + n + 64), rand_bits(rng, ro + n + 64)
            for op in range(5):
                for fill in (0x00, 0xFF):
                    init = np.full((oo + n + 7) // 8 + 9, fill, np.uint8)
                    got, exp = hip.bitmap_op(op, l, lo, r, ro, init, oo, n), orc_be.bitmap_op(op, l, lo, r, ro, init, oo, n)
                    assert got.tobytes() == exp.tobytes(), (op, n, lo, ro, oo, fill)
            assert hip.count_set_bits(l, lo, n) == orc_be.count_set_bits(l, lo, n)
            init = np.full((oo + n + 7) // 8 + 9, 0x5A, np.uint8)
            for inv in (False, True):
                assert hip.copy_bitmap(l, lo, n, init, oo, inv).tobytes() == orc_be.copy_bitmap(l, lo, n, init, oo, inv).tobytes()
            for v in (False, True):
                assert hip.set_bits_to(init, oo, n, v).tobytes() == orc_be.set_bits_to(init, oo, n, v).tobytes()


def test_kleene_random(hip, orc_be):
    rng = np.random.default_rng(34)
    for n in [1, 63, 64, 1000, 70001]:
        for lo, ro, oo in [(0, 0, 0), (3, 5, 7), (64, 1, 9)]:
            lv, ld = rand_bits(rng, lo + n + 64, 0.8), rand_bits(rng, lo + n + 64)
            rv, rd = rand_bits(rng, ro + n + 64, 0.8), rand_bits(rng, ro + n + 64)
            for op in range(3):
                for lvv, rvv in [(lv, rv), (None, rv), (lv, None)]:
                    iv = np.full((oo + n + 7) // 8 + 9, 0xFF, np.uint8); idt = np.full((oo + n + 7) // 8 + 9, 0x00, np.uint8)
                    gv, gd = hip.kleene(op, lvv, ld, lo, rvv, rd, ro, iv, idt, oo, n)
                    ev, ed = orc_be.kleene(op, lvv, ld, lo, rvv, rd, ro, iv, idt, oo, n)
                    assert gv.tobytes() == ev.tobytes() and gd.tobytes() == ed.tobytes(), (op, n, lo, ro, oo)


# ---- filter -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.int64], ids=str)
def test_filter_bit_exact(hip, orc_be, dtype):
    # random compare-then-filter (vector_selection_test.go:554-613) generalised: every
    # null combination, both NullSelection modes, non-zero bit offsets, misaligned values
    rng = np.random.default_rng(41)
    w = np.dtype(dtype).itemsize
    tile = 16384 // w
    for n in [1, 8, 63, 512, tile - 1, tile, tile + 1, 3 * tile + 17, 70001]:
        vals = rand(rng, dtype, n)
        for sel_p in (0.01, 0.5, 0.97):
            for voff, foff in [(0, 0), (3, 2), (64, 9)]:
                fdata = rand_bits(rng, foff + n + 64, sel_p)
                for vvalid, fvalid in [(None, None), (rand_bits(rng, voff + n + 64, 0.9), None),
                                       (None, rand_bits(rng, foff + n + 64, 0.9)),
                                       (rand_bits(rng, voff + n + 64, 0.9), rand_bits(rng, foff + n + 64, 0.9))]:
                    want_valid = vvalid is not None or fvalid is not None
                    for null_sel in (DROP, EMIT):
                        g = hip.filter(vals, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid, misalign=voff & 1)
                        e = orc_be.filter(vals, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid)
                        assert g[0].tobytes() == e[0].tobytes(), (dtype, n, sel_p, voff, foff, null_sel)
                        if want_valid:
                            assert g[1].tobytes() == e[1].tobytes(), (dtype, n, sel_p, voff, foff, null_sel)
                        assert g[2] == e[2]
                        assert hip.filter_count(fdata, fvalid, foff, n, null_sel) == len(e[0])


def test_filter_count_cache(ctx, orc_be):
    """ah_filter_count leaves the tile prefixes of its mask for the fill that follows (no second count).  The fill must still see
    the mask as it IS: anything that can change device memory between the two calls — an upload or a kernel writing the mask's
    bytes — drops the tables; allocation / memset of other buffers and a second fill with the same mask keep them."""
    import arrow_go_amd as ah
    N = ah._native
    rng = np.random.default_rng(45)
    n = 5 * 2048 + 77
    vals = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    vals2 = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    dv, dv2 = ctx.to_device(vals), ctx.to_device(vals2)
    bits_a = rng.random(n + 64) < 0.4
    bits_b = np.roll(bits_a[:n], 1234)                       # same number of survivors, other rows
    mask_a = np.packbits(bits_a, bitorder="little")
    mask_b = np.packbits(np.concatenate([bits_b, bits_a[n:]]), bitorder="little")
    dm = ctx.to_device(mask_a)

    def fill(values_dev, k):
        ob = ctx.alloc(k * 8 + 128)                           # alloc + memset between count and fill, as the Go executor does
        ob.memset(0xCD)
        ctx.filter_primitive(8, values_dev, None, 0, dm, None, 0, n, DROP, k, ob, None)
        r = ob.download(np.int64, k)
        ob.free()
        return r

    k = ctx.filter_count(dm, None, 0, n, DROP)
    assert k == int(bits_a[:n].sum())
    assert fill(dv, k).tobytes() == vals[bits_a[:n]].tobytes()
    assert fill(dv2, k).tobytes() == vals2[bits_a[:n]].tobytes()      # second column, same tables
    # the mask changes under the same pointer after the count: upload
    k = ctx.filter_count(dm, None, 0, n, DROP)
    dm.upload(mask_b)
    assert fill(dv, k).tobytes() == vals[bits_b].tobytes()
    # ... and by a kernel: greater(vals, 0) written over the mask
    ctx.comparison(N.CMP_GT, N.SHAPE_AS, N.INT64, dv, np.array([0], np.int64), dm, n, 0)
    gt = vals > 0
    k = ctx.filter_count(dm, None, 0, n, DROP)
    assert k == int(gt.sum())
    ctx.comparison(N.CMP_GT, N.SHAPE_AS, N.INT64, dv2, np.array([0], np.int64), dm, n, 0)   # same pointer, new content, stale tables
    gt2 = vals2 > 0
    assert fill(dv, int(gt2.sum())).tobytes() == vals[gt2].tobytes()
    # other range of the same buffer: recounted
    k = ctx.filter_count(dm, None, 0, n, DROP)
    sub = gt2[3:3 + n - 100]
    ob = ctx.alloc(n * 8 + 128)
    ctx.filter_primitive(8, dv, None, 0, dm, None, 3, n - 100, DROP, int(sub.sum()), ob, None)
    assert ob.download(np.int64, int(sub.sum())).tobytes() == vals[:n - 100][sub].tobytes()
    for b in (dv, dv2, dm, ob):
        b.free()


def test_filter_dev_flavour(hip, orc_be):
    """ah_filter_primitive_dev: no count call, worst-case outputs, {selected, nulls} left on the device — same bytes"""
    rng = np.random.default_rng(44)
    for dtype, n in [(np.int64, 1), (np.int64, 70001), (np.uint8, 40000), (np.float32, 4096 * 3 + 5)]:
        vals = rand(rng, dtype, n)
        for sel_p in (0.0, 0.3, 1.0):
            fdata = rand_bits(rng, n + 80, sel_p)
            for vvalid, fvalid, voff, foff in [(None, None, 0, 0), (rand_bits(rng, n + 80, 0.9), rand_bits(rng, n + 80, 0.9), 3, 9)]:
                want_valid = vvalid is not None
                for null_sel in (DROP, EMIT):
                    g = hip.filter_dev(vals, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid)
                    e = orc_be.filter(vals, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid)
                    assert g[0].tobytes() == e[0].tobytes(), (dtype, n, sel_p, null_sel)
                    if want_valid:
                        assert g[1].tobytes() == e[1].tobytes(), (dtype, n, sel_p, null_sel)
                    assert g[2] == e[2]


def test_take_dev_flavour(hip, orc_be):
    """ah_take_primitive_dev: same bytes, {first offending position, nulls} left on the device"""
    rng = np.random.default_rng(54)
    for vdtype, idtype, nvalues, nidx in [(np.int64, np.int32, 5000, 70001), (np.uint8, np.uint16, 300, 4099), (np.float32, np.int64, 1, 1)]:
        vals = rand(rng, vdtype, nvalues)
        idx = rng.integers(0, nvalues, nidx).astype(idtype)
        for vvalid, ivalid in [(None, None), (rand_bits(rng, nvalues + 8, 0.9), rand_bits(rng, nidx + 8, 0.9))]:
            want_valid = vvalid is not None
            g = hip.take_dev(vals, vvalid, 0, idx, ivalid, 0, want_valid)
            e = orc_be.take(vals, vvalid, 0, idx, ivalid, 0, True, want_valid)
            assert g[3] is None and g[0].tobytes() == e[1].tobytes()
            if want_valid:
                assert g[1].tobytes() == e[2].tobytes() and g[2] == e[3]
    # an out-of-range index: its position (the first one in index order, null index slots skipped) instead of an error
    vals = np.arange(1000, dtype=np.int64)
    idx = rng.integers(0, 1000, 50000).astype(np.int32)
    bad = np.sort(rng.choice(50000, 20, replace=False))
    idx[bad] = 1000 + np.arange(20)
    ivalid = rand_bits(rng, 50000, 0.7)
    assert hip.take_dev(vals, None, 0, idx, None, 0, False)[3] == bad[0]
    ok = np.unpackbits(ivalid, bitorder="little")[:50000].astype(bool)
    assert hip.take_dev(vals, None, 0, idx, ivalid, 0, True)[3] == bad[ok[bad]][0]


def test_filter_all_and_none(hip, orc_be):
    n = 40000
    vals = np.arange(n, dtype=np.int64)
    ones, zeros = np.full(n // 8 + 8, 0xFF, np.uint8), np.zeros(n // 8 + 8, np.uint8)
    out, _, _ = hip.filter(vals, None, 0, ones, None, 0, n, DROP, False)
    assert out.tobytes() == vals.tobytes()
    out, _, _ = hip.filter(vals, None, 0, zeros, None, 0, n, DROP, False)
    assert len(out) == 0
    # "runs" mask (long runs exercise whole-tile-selected and whole-tile-empty paths)
    rng = np.random.default_rng(2)
    runs = np.repeat(rng.random(n // 500 + 1) < 0.5, 500)[:n]
    fdata = OL.pack_bits(runs)
    g = hip.filter(vals, None, 0, fdata, None, 0, n, DROP, False)
    assert g[0].tobytes() == vals[runs].tobytes()


def test_filter_to_indices_random(hip, orc_be):
    rng = np.random.default_rng(43)
    for n in [1, 4095, 4096, 4097, 70001]:
        fdata, fvalid = rand_bits(rng, n + 80, 0.3), rand_bits(rng, n + 80, 0.9)
        for foff in (0, 11):
            for fv in (None, fvalid):
                for null_sel in (DROP, EMIT):
                    want_valid = fv is not None and null_sel == EMIT
                    g = hip.filter_to_indices(fdata, fv, foff, n, null_sel, want_valid)
                    e = orc_be.filter_to_indices(fdata, fv, foff, n, null_sel, want_valid)
                    assert g[0].tobytes() == e[0].tobytes()
                    if want_valid:
                        assert g[1].tobytes() == e[1].tobytes() and g[2] == e[2]


# ---- take ---------------------------------------------------------------------------------
@pytest.mark.parametrize("vdtype", [np.uint8, np.int16, np.float32, np.int64], ids=str)
@pytest.mark.parametrize("idtype", [np.int8, np.uint16, np.int32, np.uint32, np.int64, np.uint64], ids=str)
def test_take_bit_exact(hip, orc_be, vdtype, idtype):
    rng = np.random.default_rng(51)
    for nvalues, nidx in [(1, 1), (100, 63), (100, 1025), (5000, 4099), (120, 70001)]:
        hi = min(nvalues, np.iinfo(idtype).max + 1)
        vals = rand(rng, vdtype, nvalues)
        idx = rng.integers(0, hi, nidx).astype(idtype)
        for voff, ioff in [(0, 0), (5, 3)]:
            for vvalid, ivalid in [(None, None), (rand_bits(rng, voff + nvalues + 8, 0.9), None),
                                   (None, rand_bits(rng, ioff + nidx + 8, 0.9)),
                                   (rand_bits(rng, voff + nvalues + 8, 0.9), rand_bits(rng, ioff + nidx + 8, 0.9))]:
                want_valid = vvalid is not None or ivalid is not None
                g = hip.take(vals, vvalid, voff, idx, ivalid, ioff, True, want_valid)
                e = orc_be.take(vals, vvalid, voff, idx, ivalid, ioff, True, want_valid)
                assert g[0] == e[0] == STATUS_OK
                assert g[1].tobytes() == e[1].tobytes(), (vdtype, idtype, nvalues, nidx)
                if want_valid:
                    assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3]


@pytest.mark.parametrize("w", [16, 32, 3, 5, 12, 24, 100])
def test_take_wide_slots_bit_exact(hip, orc_be, w):
    """FSBImpl's take (vector_selection.go:1997-2031) for 16- and 32-byte slots — Decimal128 / Decimal256 / binary(16|32) — and for
    odd widths (binary(3) is the reference's own test column; the byte-wise kernel) through ah_take_primitive: every index type, nulls on either side, offsets, the first
    out-of-range index by value"""
    rng = np.random.default_rng(57 + w)
    vt = np.dtype(f"V{w}")
    for nvalues, nidx in [(1, 1), (100, 63), (5000, 4099), (120, 70001), (300_000, 200_003)]:
        vals = rng.integers(0, 256, (nvalues, w), dtype=np.uint8).view(vt).reshape(-1)
        for idtype in (np.int8, np.uint16, np.int32, np.uint32, np.int64, np.uint64):
            hi = min(nvalues, np.iinfo(idtype).max + 1)
            idx = rng.integers(0, hi, nidx).astype(idtype)
            for voff, ioff in [(0, 0), (5, 3)]:
                for vvalid, ivalid in [(None, None), (rand_bits(rng, voff + nvalues + 8, 0.9), rand_bits(rng, ioff + nidx + 8, 0.9))]:
                    want_valid = vvalid is not None
                    g = hip.take(vals, vvalid, voff, idx, ivalid, ioff, True, want_valid)
                    e = orc_be.take(vals, vvalid, voff, idx, ivalid, ioff, True, want_valid)
                    assert g[0] == e[0] == STATUS_OK
                    assert g[1].tobytes() == e[1].tobytes(), (w, idtype, nvalues, nidx)
                    if want_valid:
                        assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3]
    # identity, reversed and sorted-with-repeats index vectors (the shapes the 4- / 8-byte kernels special-case), after a clustered
    # 8-byte take on the same context (its neighbour sample leaves a hint behind)
    n = 300_000
    vals = rng.integers(0, 256, (n, w), dtype=np.uint8).view(vt).reshape(-1)
    small = rng.integers(0, 1 << 60, n).astype(np.int64)
    ident = np.arange(n, dtype=np.int32)
    assert hip.take(small, None, 0, ident, None, 0, True, False)[1].tobytes() == small.tobytes()
    vvalid, ivalid = rand_bits(rng, n + 8, 0.9), rand_bits(rng, n + 8, 0.9)
    for idx in (ident, ident[::-1].copy(), np.sort(rng.integers(0, n, n)).astype(np.int32)):
        for vv, iv in ((None, None), (vvalid, ivalid)):
            g = hip.take(vals, vv, 0, idx, iv, 0, True, vv is not None)
            e = orc_be.take(vals, vv, 0, idx, iv, 0, True, vv is not None)
            assert g[0] == e[0] == STATUS_OK and g[1].tobytes() == e[1].tobytes()
            if vv is not None:
                assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3]
    vals = rng.integers(0, 256, (1000, w), dtype=np.uint8).view(vt).reshape(-1)
    idx = rng.integers(0, 1000, 5000).astype(np.int32)
    idx[[4000, 777]] = [1000, -3]
    g = hip.take(vals, None, 0, idx, None, 0, True, False)
    e = orc_be.take(vals, None, 0, idx, None, 0, True, False)
    assert g[0] == e[0] == STATUS_EINDEX and g[4] == e[4] == -3


def test_take_hint_cache_stale_is_harmless(ctx, orc_be):
    """The neighbour sample that picks a Take's path (direct / 16-byte rows per lane / binned) is kept for the Take that directly follows
    with the same index vector (option take_hint_cache; the filter cache's rules).  The vector rewritten IN PLACE between two calls —
    identity → random → sorted → identity — through the library (the upload drops the entry) and BEHIND ITS BACK (a second context on
    the same device writes the bytes: the entry is stale): the results are the oracle's either way — values, validity, null count —
    as they are with the cache off."""
    rng = np.random.default_rng(61)
    nvalues, nidx = 1 << 23, 1 << 20          # 64 MiB of Int64 values, 2^20 indices: where the sample runs
    vals = rng.integers(-2**62, 2**62, nvalues)
    vvalid, ivalid = rand_bits(rng, nvalues + 8, 0.9), rand_bits(rng, nidx + 8, 0.9)
    dv, dvv, div = ctx.to_device(vals), ctx.to_device(vvalid), ctx.to_device(ivalid)
    didx = ctx.alloc(nidx * 4 + 64)
    out, ov = ctx.alloc(nidx * 8 + 64), ctx.alloc(nidx // 8 + 64)
    ident = np.arange(nidx, dtype=np.int32)
    pats = [ident, rng.integers(0, nvalues, nidx).astype(np.int32), np.sort(rng.integers(0, nvalues, nidx)).astype(np.int32), ident,
            ident[::-1].copy(), rng.integers(0, nvalues, nidx).astype(np.int32)]
    import arrow_go_amd as ah
    from arrow_go_amd._native import lib as _lib, check as _check
    other = ah.Context(0)
    try:
        for cache, foreign in ((1, False), (1, True), (0, False)):
            ctx.set_option("take_hint_cache", cache)
            for idx in pats:
                if foreign:                    # another context's upload: this one's entry is not dropped
                    _check(other.handle, _lib.ah_upload_async(other.handle, didx.ptr, idx.ctypes.data, idx.nbytes))
                    other.sync()
                else:
                    didx.upload(idx)           # the same device address every time
                for nulls in (False, True):
                    for _ in range(2):         # the second call finds the first one's entry
                        out.memset(0xCD); ov.memset(0xCD)
                        got_nulls = ctx.take_primitive(8, dv, dvv if nulls else None, 0, nvalues, 4, True, didx, div if nulls else None, 0, nidx, True,
                                                       out, ov if nulls else None)
                        e = orc_be.take(vals, vvalid if nulls else None, 0, idx, ivalid if nulls else None, 0, True, nulls)
                        assert out.download(np.int64, nidx).tobytes() == e[1].tobytes(), (cache, nulls)
                        if nulls:
                            assert ov.download(np.uint8, nidx // 8).tobytes() == e[2].tobytes() and got_nulls == e[3], (cache, nulls)
    finally:
        ctx.set_option("take_hint_cache", 1)
        other.close()


@pytest.mark.parametrize("vdtype", [np.float32, np.int64, np.uint32, np.float64])
def test_take_vec_path_bit_exact(ctx, hip, orc_be, vdtype):
    """take_vec_kernel (16 / W adjacent rows per lane; one merged 16-byte load when their indices are consecutive, ascending or
    descending), forced on for every call: identity, reversed, sorted-with-repeats, runs broken by jumps, random; nulls on either
    side with bit offsets; every index type; ragged ends; the first out-of-range index."""
    rng = np.random.default_rng(55)
    ctx.set_option("take_vec", 2)
    try:
        for nvalues, nidx in [(1, 1), (3, 2), (100, 63), (100, 1025), (5000, 4099), (70001, 70001), (300007, 131075)]:
            vals = rand(rng, vdtype, nvalues)
            base = np.arange(nidx, dtype=np.int64) % nvalues
            pats = {"identity": base, "reverse": (nvalues - 1 - base), "sorted": np.sort(rng.integers(0, nvalues, nidx)),
                    "random": rng.integers(0, nvalues, nidx)}
            runs = base.copy()
            cuts = rng.integers(0, nidx, max(1, nidx // 37))
            runs[cuts] = rng.integers(0, nvalues, cuts.size)      # consecutive runs broken at odd and even rows
            pats["broken_runs"] = runs
            pats["rev_sorted"] = np.sort(rng.integers(0, nvalues, nidx))[::-1]
            for name, ix64 in pats.items():
                for idtype in ((np.int32, np.uint64, np.int16, np.uint8) if name in ("identity", "broken_runs") else (np.int32,)):
                    hi = np.iinfo(idtype).max
                    ix = np.minimum(ix64, min(hi, nvalues - 1)).astype(idtype)
                    for voff, ioff in [(0, 0), (5, 3)]:
                        nv = nvalues - voff
                        if nv < 1:
                            continue
                        ixx = np.minimum(ix.astype(np.int64), nv - 1).astype(idtype)
                        for vvalid, ivalid in [(None, None), (rand_bits(rng, nvalues + 8, 0.9), None), (None, rand_bits(rng, ioff + nidx + 8, 0.9)),
                                               (rand_bits(rng, nvalues + 8, 0.5), rand_bits(rng, ioff + nidx + 8, 0.5))]:
                            want_valid = vvalid is not None or ivalid is not None
                            g = hip.take(vals[voff:], vvalid, voff, ixx, ivalid, ioff, True, want_valid)
                            e = orc_be.take(vals[voff:], vvalid, voff, ixx, ivalid, ioff, True, want_valid)
                            assert g[0] == e[0] == STATUS_OK
                            assert g[1].tobytes() == e[1].tobytes(), (vdtype, name, idtype, nvalues, nidx, voff)
                            if want_valid:
                                assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3], (vdtype, name, idtype, nvalues, nidx, voff)
        vals = rand(rng, vdtype, 50_000)
        idx = np.arange(60_000, dtype=np.int32) % 50_000
        bad = rng.integers(0, 60_000, 20)
        idx[bad] = rng.integers(50_000, 1 << 30, 20)
        idx[bad[::2]] *= -1
        for iv in (None, rand_bits(rng, 60_000, 0.7)):
            g = hip.take(vals, None, 0, idx, iv, 0, True, iv is not None)
            e = orc_be.take(vals, None, 0, idx, iv, 0, True, iv is not None)
            assert g[0] == e[0] == STATUS_EINDEX and g[4] == e[4]
    finally:
        ctx.set_option("take_vec", 1)


def test_take_first_bad_index_random(hip, orc_be):
    rng = np.random.default_rng(52)
    vals = np.arange(1000, dtype=np.int64)
    idx = rng.integers(0, 1000, 50000).astype(np.int32)
    bad_positions = rng.integers(0, 50000, 20)
    idx[bad_positions] = rng.integers(1000, 1 << 30, 20)
    idx[bad_positions[::2]] *= -1
    ivalid = rand_bits(rng, 50000, 0.7)
    for iv in (None, ivalid):
        g = hip.take(vals, None, 0, idx, iv, 0, True, iv is not None)
        e = orc_be.take(vals, None, 0, idx, iv, 0, True, iv is not None)
        assert g[0] == e[0] == STATUS_EINDEX and g[4] == e[4]


@pytest.mark.parametrize("vdtype", [np.uint8, np.int16, np.float32, np.int64])
def test_take_binned_path_bit_exact(ctx, hip, orc_be, vdtype):
    """the binned path (ah_take_binned.hip: bin → L2-window gather → unpermute), forced on at sizes the oracle does in
    milliseconds: every index type, nulls on either side, bit offsets, ragged last tile, skewed and empty bins, tiny windows"""
    rng = np.random.default_rng(53)
    ctx.set_option("take_binned", 2)
    try:
        for window_log2, nvalues, nidx in [(21, 300_000, 8192), (12, 70_001, 100_003), (10, 5_000, 40_000), (14, 1_000_000, 250_007)]:
            ctx.set_option("take_window_log2", window_log2)
            vals = rand(rng, vdtype, nvalues)
            for idtype in (np.int32, np.uint32, np.int64, np.uint64, np.int16, np.uint8):
                hi = min(nvalues, np.iinfo(idtype).max + 1)
                idx = rng.integers(0, hi, nidx).astype(idtype)
                if idtype == np.int32:   # skew: half the indices in one window, a stretch of empty windows
                    idx[::2] = rng.integers(0, min(hi, 300), (nidx + 1) // 2).astype(idtype)
                for voff, ioff in [(0, 0), (5, 3)]:
                    nv = nvalues - voff
                    ix = np.minimum(idx.astype(np.int64), nv - 1).astype(idtype)
                    for vvalid, ivalid in [(None, None), (rand_bits(rng, nvalues + 8, 0.9), None), (None, rand_bits(rng, ioff + nidx + 8, 0.9)),
                                           (rand_bits(rng, nvalues + 8, 0.5), rand_bits(rng, ioff + nidx + 8, 0.5))]:
                        want_valid = vvalid is not None or ivalid is not None
                        g = hip.take(vals[voff:], vvalid, voff, ix, ivalid, ioff, True, want_valid)
                        e = orc_be.take(vals[voff:], vvalid, voff, ix, ivalid, ioff, True, want_valid)
                        assert g[0] == e[0] == STATUS_OK
                        assert g[1].tobytes() == e[1].tobytes(), (vdtype, idtype, nvalues, nidx, voff, window_log2)
                        if want_valid:
                            assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3]
        # bounds: the first offender in index order, null slots not checked
        vals = rand(rng, vdtype, 50_000)
        idx = rng.integers(0, 50_000, 60_000).astype(np.int32)
        bad = rng.integers(0, 60_000, 20)
        idx[bad] = rng.integers(50_000, 1 << 30, 20)
        idx[bad[::2]] *= -1
        for iv in (None, rand_bits(rng, 60_000, 0.7)):
            g = hip.take(vals, None, 0, idx, iv, 0, True, iv is not None)
            e = orc_be.take(vals, None, 0, idx, iv, 0, True, iv is not None)
            assert g[0] == e[0] == STATUS_EINDEX and g[4] == e[4]
    finally:
        ctx.set_option("take_binned", 1)
        ctx.set_option("take_window_log2", 22)


# ---- hashing ------------------------------------------------------------------------------
@pytest.mark.parametrize("card", [1, 7, 1000, 40000])
def test_hash_encode_first_seen_order(hip, orc_be, card):
    rng = np.random.default_rng(61 + card)
    for n in [1, 63, 2049, 70001, 300007]:
        pool = rng.integers(0, 2**63, card, dtype=np.int64) * rng.choice([-1, 1], card)
        keys = pool[rng.integers(0, card, n)]
        valid = rand_bits(rng, n + 16, 0.9)
        for off, v in [(0, None), (0, valid), (7, valid)]:
            for enc in (True, False):
                g = hip.hash_encode(keys, v, off, enc)
                e = orc_be.hash_encode(keys, v, off, enc)
                assert g[0].tobytes() == e[0].tobytes(), (card, n, off, enc)
                assert g[1].tobytes() == e[1].tobytes()
                assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3]


def test_hash_encode_table_growth(hip, orc_be):
    # more than 2^21 distinct keys: forces the retry with a larger table
    n = (1 << 21) + 12345
    keys = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
    g = hip.hash_encode(keys, None, 0, False)
    assert g[0].tolist() == list(range(n)) if n < 10 else (g[0] == np.arange(n, dtype=np.int32)).all()
    assert g[2].tobytes() == keys.view(np.uint64).tobytes()


def test_hash_encode_capacity_estimates(hip, orc_be):
    # capacity planning extrapolates from a 2^21-row prefix; whatever it guesses, results are the oracle's
    rng = np.random.default_rng(67)
    n = (1 << 23) + 77
    cases = {
        "uniform 2^22": rng.integers(0, 1 << 22, n),
        # the prefix looks low-cardinality-ish, the rest is all new keys: under-estimate → overflow → retry
        "late burst": np.concatenate([rng.integers(0, 3 << 20, 1 << 22), (1 << 40) + np.arange(n - (1 << 22))]),
        "half unique": np.where(rng.random(n) < 0.5, rng.integers(0, 1000, n), (1 << 40) + np.arange(n)),
    }
    for name, k in cases.items():
        keys = (k.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
        g, e = hip.hash_encode(keys, None, 0, False), orc_be.hash_encode(keys, None, 0, False)
        assert g[0].tobytes() == e[0].tobytes(), name
        assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3], name


def test_hash_encode_voided_partition_attempt_keeps_prefix_ids(hip, orc_be):
    """automatic mode, a head that misleads WITHOUT a capacity restart afterwards: the first 2^21 rows draw from 4·10^5 keys (the look
    after 2^16 rows estimates ≈ 4·10^5 → one cut into 256 partitions), the rest bring the total to 1.8·10^6 (≈ 7000 keys per partition:
    the LDS tables overflow, the attempt voids itself AFTER its ids went home).  The global-table path carries on from row 2^16 with
    d0 ≈ 4·10^5 ≤ cap / 4 — no restart — so the slot numbers of rows [0, 2^16) must have been put back (they held the voided
    attempt's ids: wrong ids, and indices beyond the table)"""
    rng = np.random.default_rng(6701)
    n = (1 << 22) + 4321
    head = 1 << 21
    for total_keys in (1_800_000, 1_200_000):
        k = np.concatenate([rng.integers(0, 400_000, head), rng.integers(0, total_keys, n - head)])
        keys = (k.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
        valid = rand_bits(rng, n + 16, 0.95)
        for v, off, enc in ((None, 0, False), (valid, 3, True), (valid, 3, False)):
            g, e = hip.hash_encode(keys, v, off, enc), orc_be.hash_encode(keys, v, off, enc)
            assert g[0].tobytes() == e[0].tobytes(), (total_keys, off, enc)
            assert g[1].tobytes() == e[1].tobytes() and g[2].tobytes() == e[2].tobytes() and g[3] == e[3], (total_keys, off, enc)


def test_hash_encode_low_cardinality_lds_path(hip, orc_be):
    # more rows than the 2^21-row prefix and ≤ 4096 keys in it: the main pass looks keys up in LDS
    rng = np.random.default_rng(68)
    n = (1 << 22) + 1234
    valid = rand_bits(rng, n + 16, 0.9)
    for card in (1, 5, 1000, 4096, 5000):
        pool = rng.integers(-2**63, 2**63, card, dtype=np.int64)
        if card >= 5:
            pool[3] = -1  # the all-ones key has its own slot
        keys = pool[rng.integers(0, card, n)]
        for off, v in [(0, None), (5, valid)]:
            for enc in (True, False):
                g, e = hip.hash_encode(keys, v, off, enc), orc_be.hash_encode(keys, v, off, enc)
                assert g[0].tobytes() == e[0].tobytes(), (card, off, enc)
                assert g[1].tobytes() == e[1].tobytes() and g[2].tobytes() == e[2].tobytes() and g[3] == e[3]
    # keys, the all-ones key and nulls that first show up after the prefix: misses go to the global table
    keys = pool[:100][rng.integers(0, 100, n)]
    keys[3 << 20:] = rng.integers(0, 300, n - (3 << 20))
    keys[(3 << 20) + 17] = -1
    v = np.full((n + 7) // 8, 0xFF, np.uint8)
    v[(3 << 20) // 8 + 100] = 0
    for enc in (True, False):
        g, e = hip.hash_encode(keys, v, 0, enc), orc_be.hash_encode(keys, v, 0, enc)
        assert g[0].tobytes() == e[0].tobytes() and g[1].tobytes() == e[1].tobytes()
        assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3]
    # sorted keys: the probe segment misses all the time → the rest goes through the plain kernel
    n = (1 << 23) + (1 << 21) + 4321
    keys = (np.arange(n, dtype=np.int64) // 700) * 1000003
    g, e = hip.hash_encode(keys, None, 0, False), orc_be.hash_encode(keys, None, 0, False)
    assert g[0].tobytes() == e[0].tobytes() and g[2].tobytes() == e[2].tobytes()
    # group-by on top of it
    n = (1 << 22) + 99
    keys = rng.integers(0, 777, n).astype(np.int64) * 1000003
    iv = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    vvalid = rand_bits(rng, n + 8, 0.9)
    g, e = hip.hash_sum("i64", keys, None, 0, iv, vvalid, 5), orc_be.hash_sum("i64", keys, None, 0, iv, vvalid, 5)
    for a, b in zip(g[:3], e[:3]):
        assert a.tobytes() == b.tobytes()
    assert g[3] == e[3] and g[4].tobytes() == e[4].tobytes()


def test_hash_sum(hip, orc_be):
    rng = np.random.default_rng(71)
    for n, card in [(1, 1), (1000, 3), (70001, 500), (200001, 5000), (1 << 18, 9000), (300007, 100000),
                    (2500003, 1 << 21), ((1 << 22) + 5, 1 << 24)]:  # LDS · one-pass partition (4 Ki < groups ≤ 1 Mi) · two-pass partition
        keys = rng.integers(0, card, n).astype(np.int64) * 1000003
        kvalid, vvalid = rand_bits(rng, n + 8, 0.95), rand_bits(rng, n + 8, 0.9)
        iv = rng.integers(-2**62, 2**62, n, dtype=np.int64)
        g, e = hip.hash_sum("i64", keys, kvalid, 3, iv, vvalid, 5), orc_be.hash_sum("i64", keys, kvalid, 3, iv, vvalid, 5)
        for a, b in zip(g[:3], e[:3]):
            assert a.tobytes() == b.tobytes()
        assert g[3] == e[3] and g[4].tobytes() == e[4].tobytes()  # null group id, first rows
        # f64: integer-valued data → exact in any order → bit-exact vs the sequential oracle
        fv = rng.integers(-1000, 1000, n).astype(np.float64)
        g, e = hip.hash_sum("f64", keys, kvalid, 3, fv, vvalid, 5), orc_be.hash_sum("f64", keys, kvalid, 3, fv, vvalid, 5)
        for a, b in zip(g[:3], e[:3]):
            assert a.tobytes() == b.tobytes()
        # general data: tolerance n_g·ε·Σ|x| per group — the bound of the oracle's own sequential order (ours is tighter:
        # test_hash_sum_f64_is_deterministic_and_tight)
        fv = rng.uniform(-1, 1, n)
        g, e = hip.hash_sum("f64", keys, kvalid, 3, fv, vvalid, 5), orc_be.hash_sum("f64", keys, kvalid, 3, fv, vvalid, 5)
        assert g[0].tobytes() == e[0].tobytes() and g[2].tobytes() == e[2].tobytes()
        tol = np.maximum(e[2], 1) * 2.3e-16 * np.maximum(e[2], 1)  # n_g·ε·(Σ|x| ≤ n_g)
        assert (np.abs(g[1] - e[1]) <= tol).all()


def _hash_sum_cases(rng, n, card, hot=0.0):
    keys = rng.integers(0, card, n).astype(np.int64) * 1000003
    if hot:
        keys[rng.random(n) < hot] = 7 * 1000003          # one key owns a large share of the rows (chunks of one partition)
    keys[rng.integers(0, n, 5)] = -1                       # the all-ones key: the tables' EMPTY marker
    kvalid, vvalid = rand_bits(rng, n + 8, 0.95), rand_bits(rng, n + 8, 0.9)
    return keys, kvalid, vvalid


@pytest.mark.parametrize("n,card,mode,hot", [
    (70001, 500, -2, 0.0),         # no cut: chunks of the columns aggregated in LDS, merged into one global table
    (3000017, 1500, -2, 0.6),      # … with a hot key and a dozen chunks
    (3000017, 9000, -2, 0.0),      # … and more keys than the LDS table admits: the rest goes straight to the global table
    (70001, 500, 5, 0.0),          # 8 partitions of one chunk each: the LDS table leaves as a copy
    (300007, 20000, 5, 0.0),
    (6000017, 9000, 5, 0.6),       # a hot key: its partition is cut into chunks, merged into the global table; runs combined per lane
    (1 << 21, 48000, 5, 0.0),      # 6000 keys per partition: beyond the LDS table's 3584 → later keys go to the global table
    (1 << 21, 160000, 5, 0.0),     # 20000 keys per partition: the global table overflows → the id-based path answers
    (2500003, 700000, 12, 0.0),    # 1024 partitions
    ((1 << 22) + 77, 1 << 21, 3, 0.0),     # 2048 partitions through the two-level cut, one workgroup per partition
    ((1 << 22) + 77, 1 << 22, 4, 0.0),     # 8192 partitions
    ((1 << 22) + 77, 1 << 24, 3, 0.0),     # far more keys per partition than an LDS table holds → the id-based path answers
    ((1 << 22) + 77, 3 << 20, 2, 0.0),     # very many groups: sort-based buckets (ah_groupby.hip gs_*), one wave per bucket
    ((1 << 22) + 77, 1 << 24, 2, 0.0),     # nearly every row its own group
    ((1 << 22) + 77, 1 << 21, 2, 0.01),    # a key with 40 000 rows among two million groups: its bucket is beyond a wave → the id-based path answers
])
def test_hash_sum_partition_first(hip, orc_be, ctx, n, card, mode, hot):
    """ah_groupby.hip: rows cut by key hash, each partition aggregated in LDS.  Same bytes as the id-based path and as the
    oracle (ids = first-seen order, int sums wrap, integer-valued float sums exact, counts, first rows, null group)."""
    rng = np.random.default_rng(n + card)
    keys, kvalid, vvalid = _hash_sum_cases(rng, n, card, hot)
    iv = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    fi = rng.integers(-1000, 1000, n).astype(np.float64)
    # 35 binades: inside the 42 one fixed-point scale holds exactly, so the partition-first passes keep the call (a wider column is
    # handed to the id-based path and its per-group scales: test_hash_sum_f64_wide_range)
    fv = (1.0 + rng.random(n)) * np.exp(rng.uniform(-12, 12, n)) * rng.choice([-1.0, 1.0], n)
    fv[rng.integers(0, n, 3)] = np.inf
    fv[rng.integers(0, n, 2)] = -np.inf
    fv[rng.integers(0, n, 2)] = np.nan
    try:
        ctx.set_option("groupby_partition", 0)
        base = {k: hip.hash_sum(k[0:3], keys, kvalid, 3, v, vvalid, 5) for k, v in (("i64", iv), ("f64i", fi), ("f64v", fv))}
        ctx.set_option("groupby_partition", mode)
        got = {k: hip.hash_sum(k[0:3], keys, kvalid, 3, v, vvalid, 5) for k, v in (("i64", iv), ("f64i", fi), ("f64v", fv))}
        again = hip.hash_sum("f64", keys, kvalid, 3, fv, vvalid, 5)
    finally:
        ctx.set_option("groupby_partition", 1)
    for k in got:
        g, b = got[k], base[k]
        assert g[0].tobytes() == b[0].tobytes() and g[1].tobytes() == b[1].tobytes() and g[2].tobytes() == b[2].tobytes(), k
        assert g[3] == b[3] and g[4].tobytes() == b[4].tobytes(), k
    assert again[1].tobytes() == got["f64v"][1].tobytes()
    for k, v in (("i64", iv), ("f64i", fi)):
        e = orc_be.hash_sum(k[0:3], keys, kvalid, 3, v, vvalid, 5)
        g = got[k]
        for a, b in zip(g[:3], e[:3]):
            assert a.tobytes() == b.tobytes(), k
        assert g[3] == e[3] and g[4].tobytes() == e[4].tobytes(), k


@pytest.mark.parametrize("mode,card", [(3, 1 << 21), (4, 1 << 22), (4, 3 << 20)])
def test_hash_sum_two_level_reserving(hip, orc_be, ctx, mode, card):
    """Round 6, the two-level cut (2048 … 8192 partitions) without key nulls: the second level's scatter RESERVES its runs in fixed
    regions, one per final partition (gs_scatter_kernel RES: no histogram of the first level's output), and the groups leave the LDS
    tables as 32-byte records binned by first row (GbRec) — ids from a per-bin bitmap in LDS.  Same bytes as the id-based path and as
    the oracle, run to run; a key with tens of thousands of rows overflows its partition's region: the attempt is void and the level
    is run again behind a histogram (option groupby_reserve 0 takes that way from the start: the same bytes again)."""
    rng = np.random.default_rng(4242 + mode + card % 97)
    n = (1 << 22) + 77
    for hot in (0.0, 0.02):
        keys = rng.integers(0, card, n).astype(np.int64) * 1000003
        if hot:
            keys[rng.random(n) < hot] = 7 * 1000003
        keys[rng.integers(0, n, 5)] = -1                       # the all-ones key: the tables' EMPTY marker
        vvalid = rand_bits(rng, n + 8, 0.9)
        iv = rng.integers(-2**62, 2**62, n, dtype=np.int64)
        fv = (1.0 + rng.random(n)) * np.exp(rng.uniform(-12, 12, n)) * rng.choice([-1.0, 1.0], n)
        fv[rng.integers(0, n, 3)] = np.inf
        fv[rng.integers(0, n, 2)] = np.nan
        res = {}
        try:
            ctx.set_option("groupby_partition", 0)
            res["ids"] = [hip.hash_sum(k, keys, None, 0, v, vvalid, 5) for k, v in (("i64", iv), ("f64", fv))]
            ctx.set_option("groupby_partition", mode)
            res["reserve"] = [hip.hash_sum(k, keys, None, 0, v, vvalid, 5) for k, v in (("i64", iv), ("f64", fv))]
            again = hip.hash_sum("f64", keys, None, 0, fv, vvalid, 5)
            ctx.set_option("groupby_reserve", 0)
            res["hist"] = [hip.hash_sum(k, keys, None, 0, v, vvalid, 5) for k, v in (("i64", iv), ("f64", fv))]
        finally:
            ctx.set_option("groupby_partition", 1)
            ctx.set_option("groupby_reserve", 1)
        for variant in ("reserve", "hist"):
            for g, b in zip(res[variant], res["ids"]):
                assert g[0].tobytes() == b[0].tobytes() and g[2].tobytes() == b[2].tobytes(), (variant, hot, "keys / counts")
                assert same_bits_or_both_nan(g[1], b[1]), (variant, hot, "sums")
                assert g[3] == b[3] and g[4].tobytes() == b[4].tobytes(), (variant, hot)
        assert again[1].tobytes() == res["reserve"][1][1].tobytes(), "run to run"
        e = orc_be.hash_sum("i64", keys, None, 0, iv, vvalid, 5)
        g = res["reserve"][0]
        for a, b in zip(g[:3], e[:3]):
            assert a.tobytes() == b.tobytes()
        assert g[3] == e[3] and g[4].tobytes() == e[4].tobytes()


@pytest.mark.parametrize("hot", [0.0, 0.02])
def test_hash_sum_two_level_auto(hip, orc_be, ctx, hot):
    """the two-level cut as the dispatcher reaches it (option groupby_partition 1): 2^23 rows over 3·2^20 evenly drawn keys — the 2^21-row
    sample says ≈ 3 M groups and leaves its [8][1024] histogram, so the FIRST level is the one-level cut's reserving scatter (a region per
    parent and XCD, gb_scatter_kernel RESERVE) and the second level tiles those regions (gs_subregions_kernel); with a key that owns 2 % of
    the rows a final partition's region overflows and the level runs again behind a histogram.  Bytes of the id-based path and the oracle."""
    rng = np.random.default_rng(2323 + int(hot * 100))
    n = (1 << 23) + 77
    keys = rng.integers(0, 3 << 20, n).astype(np.int64) * 1000003
    if hot:
        keys[rng.random(n) < hot] = 7 * 1000003
    vvalid = rand_bits(rng, n + 8, 0.9)
    iv = rng.integers(-2**62, 2**62, n, dtype=np.int64)
    fv = (1.0 + rng.random(n)) * np.exp(rng.uniform(-12, 12, n)) * rng.choice([-1.0, 1.0], n)
    try:
        ctx.set_option("groupby_partition", 0)
        base = [hip.hash_sum(k, keys, None, 0, v, vvalid, 5) for k, v in (("i64", iv), ("f64", fv))]
    finally:
        ctx.set_option("groupby_partition", 1)
    got = [hip.hash_sum(k, keys, None, 0, v, vvalid, 5) for k, v in (("i64", iv), ("f64", fv))]
    again = hip.hash_sum("f64", keys, None, 0, fv, vvalid, 5)
    for g, b in zip(got, base):
        assert g[0].tobytes() == b[0].tobytes() and g[1].tobytes() == b[1].tobytes() and g[2].tobytes() == b[2].tobytes()
        assert g[3] == b[3] and g[4].tobytes() == b[4].tobytes()
    assert again[1].tobytes() == got[1][1].tobytes()
    e = orc_be.hash_sum("i64", keys, None, 0, iv, vvalid, 5)
    for a, b in zip(got[0][:3], e[:3]):
        assert a.tobytes() == b.tobytes()
    assert got[0][3] == e[3] and got[0][4].tobytes() == e[4].tobytes()


@pytest.mark.parametrize("mode", [5, 8, 11, 12])
def test_hash_sum_reserving_scatter(hip, orc_be, ctx, mode):
    """ah_partition.h 1b: the scatter that reserves its runs in per-(partition, XCD) regions sized from the key sample (option
    groupby_reserve, the default) against the histogram → offsets → scatter pipeline: the same bytes, on evenly spread keys, with a hot
    key and null keys (partition 0), and on a column whose hot key the sample CANNOT see in proportion — every sampled row (64 of each
    256) avoids it — so that its region overflows, the attempt is void and the call is redone with the histogram."""
    rng = np.random.default_rng(900 + mode)
    n = (1 << 23) + 4321
    cases = []
    keys, kvalid, vvalid = _hash_sum_cases(rng, n, 40000 if mode < 11 else 900000, 0.0)
    cases.append(("even", keys, kvalid, vvalid))
    keys, kvalid, vvalid = _hash_sum_cases(rng, n, 40000 if mode < 11 else 900000, 0.3)
    cases.append(("hot", keys, kvalid, vvalid))
    keys, kvalid, vvalid = _hash_sum_cases(rng, n, 40000 if mode < 11 else 900000, 0.0)
    hidden = (np.arange(n) % 256 >= 64) & (np.arange(n) < (1 << 20))      # the sample reads rows g·256 … g·256 + 63
    keys[hidden] = 11 * 1000003
    cases.append(("hidden hot key", keys, kvalid, vvalid))
    for name, keys, kvalid, vvalid in cases:
        iv = rng.integers(-2**62, 2**62, n, dtype=np.int64)
        fv = (1.0 + rng.random(n)) * np.exp(rng.uniform(-12, 12, n)) * rng.choice([-1.0, 1.0], n)
        res = {}
        try:
            ctx.set_option("groupby_partition", mode)
            for reserve in (0, 1):
                ctx.set_option("groupby_reserve", reserve)
                res[reserve] = [hip.hash_sum(k, keys, kvalid, 3, v, vvalid, 5) for k, v in (("i64", iv), ("f64", fv))]
            again = hip.hash_sum("f64", keys, kvalid, 3, fv, vvalid, 5)
        finally:
            ctx.set_option("groupby_partition", 1)
            ctx.set_option("groupby_reserve", 1)
        for a, b in zip(res[0], res[1]):
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes(), (name, mode)
            assert a[3] == b[3] and a[4].tobytes() == b[4].tobytes(), (name, mode)
        assert again[1].tobytes() == res[1][1][1].tobytes(), (name, mode)      # run to run
        e = orc_be.hash_sum("i64", keys, kvalid, 3, iv, vvalid, 5)
        g = res[1][0]
        for a, b in zip(g[:3], e[:3]):
            assert a.tobytes() == b.tobytes(), (name, mode)
        assert g[3] == e[3] and g[4].tobytes() == e[4].tobytes(), (name, mode)


def test_hash_sum_partition_first_auto(hip, orc_be):
    """the automatic choice (≥ 2^21 rows; partitions from a sampled distinct estimate), skewed keys included"""
    rng = np.random.default_rng(77)
    n = (1 << 22) + 77
    for card, zipf in [(300, False), (50000, False), (1 << 20, True), (1 << 23, False)]:
        if zipf:
            keys = (rng.zipf(1.1, n) % card).astype(np.int64) * 1000003
        else:
            keys = rng.integers(0, card, n).astype(np.int64) * 1000003
        kvalid, vvalid = rand_bits(rng, n + 8, 0.95), rand_bits(rng, n + 8, 0.9)
        iv = rng.integers(-2**62, 2**62, n, dtype=np.int64)
        g, e = hip.hash_sum("i64", keys, kvalid, 3, iv, vvalid, 5), orc_be.hash_sum("i64", keys, kvalid, 3, iv, vvalid, 5)
        for a, b in zip(g[:3], e[:3]):
            assert a.tobytes() == b.tobytes()
        assert g[3] == e[3] and g[4].tobytes() == e[4].tobytes()
        fi = rng.integers(-1000, 1000, n).astype(np.float64)
        g, e = hip.hash_sum("f64", keys, kvalid, 3, fi, vvalid, 5), orc_be.hash_sum("f64", keys, kvalid, 3, fi, vvalid, 5)
        for a, b in zip(g[:3], e[:3]):
            assert a.tobytes() == b.tobytes()


def test_hash_encode_repacked_table(hip, orc_be, ctx):
    """dictionary_encode beyond the 2^21-row prefix with 4 Ki < keys ≤ 1 Mi: the main pass probes the re-packed
    (key → id) table; keys the prefix did not hold still get their first-seen ids"""
    rng = np.random.default_rng(78)
    n = (1 << 22) + 1001
    for card in (6000, 70000, 400000):
        keys = rng.integers(0, card, n).astype(np.int64) * 1000003
        keys[(1 << 21) + 5:(1 << 21) + 5000] = np.arange(4995) + (1 << 40)     # new keys after the prefix
        keys[n - 3] = -1
        valid = rand_bits(rng, n + 8, 0.97)
        for enc in (False, True):
            g, e = hip.hash_encode(keys, valid, 3, enc), orc_be.hash_encode(keys, valid, 3, enc)
            assert g[2].size == e[2].size and g[3] == e[3], (card, enc, g[2].size, e[2].size, g[3], e[3])
            bad = np.flatnonzero(g[0] != e[0])
            assert bad.size == 0, (card, enc, bad.size, bad[:5], g[0][bad[:5]], e[0][bad[:5]])
            bits = lambda a: np.unpackbits(a, bitorder="little")[:n]    # the bits past n belong to the caller's buffer
            assert (bits(g[1]) == bits(e[1])).all() and g[2].tobytes() == e[2].tobytes(), (card, enc)
        try:
            ctx.set_option("hash_direct", 3)
            g3 = hip.hash_encode(keys, valid, 3, True)
        finally:
            ctx.set_option("hash_direct", 2)
        g2 = hip.hash_encode(keys, valid, 3, True)
        assert g3[0].tobytes() == g2[0].tobytes() and g3[2].tobytes() == g2[2].tobytes()



def _exact_group_sums(keys, fv, ok, limit):
    """{key: (Fraction exact sum of the valid values, count, max |x|)} for the first `limit` keys in sorted-key order"""
    from fractions import Fraction
    order = np.argsort(keys, kind="stable")
    ks, vs, oks = keys[order], fv[order], ok[order]
    bounds = np.flatnonzero(np.diff(ks)) + 1
    starts, ends = np.concatenate([[0], bounds])[:limit], np.concatenate([bounds, [keys.size]])[:limit]
    out = {}
    for a, b in zip(starts, ends):
        vals = vs[a:b][oks[a:b]]
        fin = vals[np.isfinite(vals)]
        out[int(ks[a])] = (sum((Fraction(float(v)) for v in fin), Fraction(0)), len(vals), float(np.abs(fin).max()) if fin.size else 0.0)
    return out


@pytest.mark.parametrize("lp", [3, 8, 10, 11, 13])   # 11, 13: two cuts (64 parents × 32 / 128), for inputs of ≥ 2^20 rows
def test_hash_encode_partitioned(hip, orc_be, ctx, lp):
    """ah_hash_part.hip (rows cut by key hash, one LDS table per partition, ids sent back to row order), forced on at sizes the
    oracle does in a second: ids, index validity, dictionary and null id byte-equal to the sequential memo table — nulls encoded
    and masked, the all-ones key, bit offsets, ragged last tile, partitions with no rows, more keys than a partition's table
    admits (the attempt is void, the global-table path answers), one key owning half the rows (not attempted)."""
    rng = np.random.default_rng(700 + lp)
    try:
        ctx.set_option("encode_partition", lp)
        for n, card, hot in [(1, 1, 0), (4096, 7, 0), (4097, 3000, 0), (70001, 500, 0), (300007, 40000, 0), ((1 << 20) + 3, 1 << 19, 0),
                             ((1 << 21) + 77, (1 << 21) + 77, 0), (500009, 20000, 0.5)]:
            keys = rng.integers(0, card, n).astype(np.int64) * 1000003
            if hot:
                keys[rng.random(n) < hot] = 12345
            if n > 10:
                keys[rng.integers(0, n, 3)] = -1          # the all-ones key
            for valid, off in ((None, 0), (rand_bits(rng, n + 16, 0.9), 5)):
                for enc in (False, True):
                    g, e = hip.hash_encode(keys, valid, off, enc), orc_be.hash_encode(keys, valid, off, enc)
                    assert g[2].size == e[2].size and g[3] == e[3], (n, card, enc, g[2].size, e[2].size, g[3], e[3])
                    bad = np.flatnonzero(g[0] != e[0])
                    assert bad.size == 0, (n, card, enc, bad.size, bad[:5], g[0][bad[:5]], e[0][bad[:5]])
                    bits = lambda a: np.unpackbits(a, bitorder="little")[:n]
                    assert (bits(g[1]) == bits(e[1])).all() and g[2].tobytes() == e[2].tobytes(), (n, card, enc)
            # unique: no ids wanted — the dictionary alone
            kb = ctx.to_device(keys.view(np.uint64)); db = ctx.alloc((n + 1) * 8 + 64)
            nd, nid = ctx.hash_u64_encode(kb, None, 0, n, True, None, None, db)
            e = orc_be.hash_encode(keys, None, 0, True)
            assert nd == e[2].size and db.download(np.uint64, nd).tobytes() == e[2].tobytes()
            kb.free(); db.free()
    finally:
        ctx.set_option("encode_partition", 1)


def _assert_encode_equals_oracle(hip, orc_be, keys, valid, off, enc, what):
    n = keys.size
    g, e = hip.hash_encode(keys, valid, off, enc), orc_be.hash_encode(keys, valid, off, enc)
    assert g[2].size == e[2].size and g[3] == e[3], (what, g[2].size, e[2].size, g[3], e[3])
    bad = np.flatnonzero(g[0] != e[0])
    assert bad.size == 0, (what, bad.size, bad[:5], g[0][bad[:5]], e[0][bad[:5]])
    bits = lambda a: np.unpackbits(a, bitorder="little")[:n]
    assert (bits(g[1]) == bits(e[1])).all() and g[2].tobytes() == e[2].tobytes(), what


@pytest.mark.parametrize("group", [1, 2, 4, 8])
def test_hash_encode_unpermute_group(hip, orc_be, ctx, group):
    """the final un-permute of the partition-first encode over 1, 2, 4 or 8 consecutive tiles per workgroup (option encode_unperm_group;
    enc_unpermute_group_kernel<G>): six tiles — for every G the last group is short of tiles and the last tile short of rows — and a
    second tile of one row; the all-ones key, a validity bitmap at bit offset 5, nulls encoded and masked.  Byte-equal to the
    sequential memo table."""
    rng = np.random.default_rng(1300 + group)
    try:
        ctx.set_option("encode_partition", 8)
        ctx.set_option("encode_unperm_group", group)
        for n in (5 * 4096 + 3, 4096 + 1):
            keys = rng.integers(0, 3000, n).astype(np.int64) * 1000003
            keys[rng.integers(0, n, 3)] = -1          # the all-ones key
            for valid, off in ((None, 0), (rand_bits(rng, n + 16, 0.9), 5)):
                for enc in (False, True):
                    _assert_encode_equals_oracle(hip, orc_be, keys, valid, off, enc, (group, n, valid is not None, enc))
    finally:
        ctx.set_option("encode_partition", 1)
        ctx.set_option("encode_unperm_group", 4)


@pytest.mark.parametrize("lp", [11, 13])
@pytest.mark.parametrize("group2", [0, 4])
def test_hash_encode_unpermute2_group(hip, orc_be, ctx, group2, lp):
    """the level-2 un-permute of the two-cut encode, one virtual tile per workgroup (option encode_unperm2_group = 0:
    e2_unpermute_kernel) or four (e2_unpermute_group_kernel<4>), at the smallest length the two-cut path accepts plus a tile and three
    rows: every parent's last virtual tile is short.  Byte-equal to the sequential memo table."""
    rng = np.random.default_rng(1400 + lp + group2)
    n = (1 << 20) + 4096 + 3
    try:
        ctx.set_option("encode_partition", lp)
        ctx.set_option("encode_unperm2_group", group2)
        keys = rng.integers(0, 1 << 19, n).astype(np.int64) * 1000003
        keys[rng.integers(0, n, 3)] = -1
        for valid, off in ((None, 0), (rand_bits(rng, n + 16, 0.9), 5)):
            for enc in (False, True):
                _assert_encode_equals_oracle(hip, orc_be, keys, valid, off, enc, (group2, lp, valid is not None, enc))
    finally:
        ctx.set_option("encode_partition", 1)
        ctx.set_option("encode_unperm2_group", 4)


@pytest.mark.parametrize("lp,byte_map", [(8, 2), (8, 0), (11, 1), (11, 0)])
def test_hash_encode_first_occurrence_marks(hip, orc_be, ctx, lp, byte_map):
    """the first-occurrence bitmap of the partition-first encode, both ways (option encode_byte_map): one device-scope atomicOr per key on
    the bitmap's words, or a plain byte store per key into a byte map that enc_bytes_to_bits_kernel packs (round 6: at 2^24 keys the
    2^24 read-modify-writes cost ≈ 0.2 ms of 2.7) — the same ids, dictionary and null id as the sequential memo table, for a length that
    ends inside a bitmap word and inside a 64-byte group of the map"""
    rng = np.random.default_rng(900 + lp + byte_map)
    try:
        ctx.set_option("encode_partition", lp)
        ctx.set_option("encode_byte_map", byte_map)
        for n, card in (((1 << 20) + 37, 1 << 19), ((1 << 21) + 77, (1 << 21) + 77)):
            keys = rng.integers(0, card, n).astype(np.int64) * 1000003
            keys[rng.integers(0, n, 3)] = -1
            valid = rand_bits(rng, n + 16, 0.9)
            for enc in (False, True):
                g, e = hip.hash_encode(keys, valid, 5, enc), orc_be.hash_encode(keys, valid, 5, enc)
                assert g[2].size == e[2].size and g[3] == e[3] and g[0].tobytes() == e[0].tobytes() and g[2].tobytes() == e[2].tobytes(), (n, enc)
    finally:
        ctx.set_option("encode_partition", 1)
        ctx.set_option("encode_byte_map", 1)


def test_hash_encode_partitioned_auto(hip, orc_be, ctx):
    """the automatic choice: ≥ 2^22 rows and a prefix that promises between encode_part_min and 4.5 M keys"""
    rng = np.random.default_rng(79)
    n = (1 << 22) + 1001
    try:
        ctx.set_option("encode_part_min", 50000)
        for card in (70000, 1 << 20):
            keys = rng.integers(0, card, n).astype(np.int64) * 1000003
            valid = rand_bits(rng, n + 8, 0.97)
            for enc in (False, True):
                g, e = hip.hash_encode(keys, valid, 3, enc), orc_be.hash_encode(keys, valid, 3, enc)
                assert g[2].size == e[2].size and g[3] == e[3] and g[0].tobytes() == e[0].tobytes() and g[2].tobytes() == e[2].tobytes(), (card, enc)
    finally:
        ctx.set_option("encode_part_min", 300000)


def test_hash_sum_f64_is_deterministic_and_tight(hip, orc_be):
    """Float64 group sums are accumulated in 128-bit fixed point with integer atomics (associative), rounded once: the bytes
    do not change from run to run.  A column spanning ≤ 42 binades keeps every addend whole, so each group's sum is the
    CORRECTLY ROUNDED exact sum; a wider column gets one scale per group and stays within ½ulp + n_g·2^-93·max_g|x| — the
    group's OWN maximum — of the exact sum, far inside the sequential definition's n_g·ε·Σ_g|x|.  ±inf / NaN addends give the
    IEEE class any order would give."""
    import math
    from fractions import Fraction
    rng = np.random.default_rng(72)
    for n, card in [(70001, 500), (300007, 100000), (2500003, 1 << 21)]:   # LDS path · one-pass partition · two-pass partition
        keys = rng.integers(0, card, n).astype(np.int64) * 1000003
        vvalid = rand_bits(rng, n + 8, 0.9)
        ok = np.unpackbits(vvalid, bitorder="little")[:n].astype(bool)
        for spread, exact_bytes in ((12, True), (30, False)):               # 35 binades (one scale, exact) · 87 binades (per-group scales)
            fv = (1.0 + rng.random(n)) * np.exp(rng.uniform(-spread, spread, n)) * rng.choice([-1.0, 1.0], n)
            runs = [hip.hash_sum("f64", keys, None, 0, fv, vvalid, 0) for _ in range(3)]
            for r in runs[1:]:
                assert r[1].tobytes() == runs[0][1].tobytes() and r[2].tobytes() == runs[0][2].tobytes()
            e = orc_be.hash_sum("f64", keys, None, 0, fv, vvalid, 0)
            g = runs[0]
            assert g[0].tobytes() == e[0].tobytes() and g[2].tobytes() == e[2].tobytes()
            pos = {int(k): i for i, k in enumerate(g[0].view(np.int64))}
            for k, (exact, cnt, gmax) in _exact_group_sums(keys, fv, ok, 2000).items():
                got = float(g[1][pos[k]])
                if exact_bytes:
                    assert got == float(exact), (n, card, k, got, float(exact))       # float(Fraction) rounds to nearest even
                else:
                    assert abs(Fraction(got) - exact) <= Fraction(0.5 * math.ulp(got)) + Fraction(gmax) * cnt / 2**93, (n, card, got, float(exact))
    # non-finite addends
    keys = np.array([1, 1, 2, 2, 3, 3, 4, 4, 5], np.int64)
    fv = np.array([np.inf, 1.0, -np.inf, 5.0, np.inf, -np.inf, np.nan, 1.0, 2.5])
    g, e = hip.hash_sum("f64", keys, None, 0, fv, None, 0), orc_be.hash_sum("f64", keys, None, 0, fv, None, 0)
    assert g[0].tobytes() == e[0].tobytes()
    assert g[1][0] == np.inf and g[1][1] == -np.inf and np.isnan(g[1][2]) and np.isnan(g[1][3]) and g[1][4] == 2.5
    assert np.array_equal(np.isnan(g[1]), np.isnan(e[1])) and np.array_equal(g[1][~np.isnan(g[1])], e[1][~np.isnan(e[1])])


@pytest.mark.parametrize("mode", [0, 1, -2, 6, 10])
def test_hash_sum_f64_wide_range(hip, orc_be, ctx, mode):
    """One outlier must not cost the other groups their sums (round-2 review, ah_hashing.h): a 1e300 sentinel in ONE group next to
    groups of ordinary values.  With one fixed-point scale for the call every addend below 2^(emax − 94) would truncate to zero;
    the call is answered with per-group scales instead.  Per-group tolerance against the exact sums, on every route
    (id-based, automatic, no-cut, 16 and 256 partitions)."""
    import math
    from fractions import Fraction
    rng = np.random.default_rng(91 + mode)
    n = (1 << 21) + 1234
    for card in (7, 3000, 100000):
        keys = rng.integers(0, card, n).astype(np.int64) * 1000003
        fv = rng.uniform(-1.0, 1.0, n)
        fv[rng.integers(0, n, 40)] = 0.0
        hot = rng.integers(0, n, 3)
        fv[hot] = [1e300, -3e299, 1.5e307]
        keys[hot] = keys[hot[0]]                       # the outliers share one group
        tiny = rng.integers(0, n, 5)
        fv[tiny] = 4.9e-324                            # denormals in other groups
        vvalid = rand_bits(rng, n + 8, 0.9)
        ok = np.unpackbits(vvalid, bitorder="little")[5:5 + n].astype(bool)
        try:
            ctx.set_option("groupby_partition", mode)
            g = hip.hash_sum("f64", keys, None, 0, fv, vvalid, 5)
            again = hip.hash_sum("f64", keys, None, 0, fv, vvalid, 5)
        finally:
            ctx.set_option("groupby_partition", 1)
        e = orc_be.hash_sum("f64", keys, None, 0, fv, vvalid, 5)
        assert g[0].tobytes() == e[0].tobytes() and g[2].tobytes() == e[2].tobytes() and g[1].tobytes() == again[1].tobytes()
        pos = {int(k): i for i, k in enumerate(g[0].view(np.int64))}
        for k, (exact, cnt, gmax) in _exact_group_sums(keys, fv, ok, 3000).items():
            got = float(g[1][pos[k]])
            assert abs(Fraction(got) - exact) <= Fraction(0.5 * math.ulp(got)) + Fraction(gmax) * cnt / 2**93, (mode, card, k, got, float(exact))
            if gmax <= 1.0 and cnt > 3:
                assert got != 0.0 or exact == 0, (mode, card, k)   # what the one-scale version returned for every ordinary group


@pytest.mark.parametrize("seed,lean", [(1, 1), (1, 0), (1, 2), (0, 1), (0, 2)])
def test_hash_sum_direct_path_seeded_tables(hip, orc_be, ctx, seed, lean):
    """The direct group-by (few groups, ≥ 2^21 rows; csrc/ah_groupby.hip): a quick look over 2^14 spread rows builds the key table every
    workgroup STARTS from (option groupby_seed), so a seeded key has one slot everywhere and the workgroups' results are added up slot
    by slot; keys the look did not see — here: keys that occur only in a few late rows, the all-ones key, the null key — take the
    atomic merge into the global table; the pending-group registers are left out when neighbouring rows rarely share a key
    (groupby_lean).  Every combination must give the oracle's groups, counts, first rows, null group and (integer-valued, exact in any
    order) sums, byte for byte, run to run."""
    rng = np.random.default_rng(2024)
    n = (1 << 22) + 4099
    for variant in ("uniform", "late keys", "runs"):
        k = rng.integers(0, 700, n).astype(np.int64)
        if variant == "late keys":
            k[n - 5000:] = 10_000 + rng.integers(0, 300, 5000)       # 300 keys no sampled row holds: they are placed behind the seeded ones
            k[n - 2] = -1                                             # the all-ones key, once
        if variant == "runs":
            k = np.repeat(rng.integers(0, 700, n // 4096 + 1), 4096)[:n].astype(np.int64)   # a lane's consecutive rows (1024 apart) mostly share a key
        keys = (k.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64) if variant != "late keys" else k
        vals = rng.integers(-2**20, 2**20, n).astype(np.float64)
        vals[rng.integers(0, n, 20)] = np.inf
        vals[rng.integers(0, n, 5)] = np.nan
        kvalid = rand_bits(rng, n + 16, 0.97)
        vvalid = rand_bits(rng, n + 16, 0.9)
        try:
            ctx.set_option("groupby_seed", seed)
            ctx.set_option("groupby_lean", lean)
            g = hip.hash_sum("f64", keys, kvalid, 5, vals, vvalid, 3)
            again = hip.hash_sum("f64", keys, kvalid, 5, vals, vvalid, 3)
            gi = hip.hash_sum("i64", keys, kvalid, 5, vals.astype(np.int64, copy=False) if False else rng.integers(-2**40, 2**40, n, dtype=np.int64), None, 0)
        finally:
            ctx.set_option("groupby_seed", 1)
            ctx.set_option("groupby_lean", 1)
        e = orc_be.hash_sum("f64", keys, kvalid, 5, vals, vvalid, 3)
        assert g[3] == e[3], (variant, "null group")
        for i, what in ((0, "group keys"), (2, "counts"), (4, "first rows")):
            assert g[i].tobytes() == e[i].tobytes(), (variant, what)
        assert same_bits_or_both_nan(g[1], e[1]), (variant, "sums")
        assert g[1].tobytes() == again[1].tobytes(), (variant, "run to run")
        assert gi[0].tobytes() == e[0].tobytes(), (variant, "int64 group keys")


@pytest.mark.parametrize("dtype", [np.int64, np.uint64, np.int32, np.uint32, np.int16, np.uint16], ids=str)
def test_cumulative_sum_one_pass(hip, orc_be, ctx, dtype):
    """cumulative_sum of unchecked 2- / 4- / 8-byte integers without nulls takes ONE pass (decoupled look-back over 128 KiB tiles,
    csrc/ah_scan.hip scan_onepass_kernel) from 2^18 rows on: sizes around the tile size (16 384 Int64 / 32 768 Int32 rows), more tiles than
    one look-back window (64) and than one generation of resident workgroups (256), a start value, wrap-around — all byte-equal to the
    sequential oracle and to the reduce-then-scan path (option scan_onepass 0), and the same bytes call after call (the record array is
    never cleared: epochs)."""
    rng = np.random.default_rng(31)
    info = np.iinfo(dtype)
    tile = 1024 * 8 * (16 // np.dtype(dtype).itemsize)
    for n in (1 << 18, (1 << 18) + 1, 17 * tile - 1, 17 * tile, 17 * tile + 1, 70 * tile + 123, 300 * tile + 7, (1 << 23) + 5):
        a = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
        start = dtype(rng.integers(info.min, info.max, dtype=dtype))
        e = orc_be.cumulative_sum(a, None, 0, start=start)
        try:
            g = hip.cumulative_sum(a, None, 0, start=start)
            g2 = hip.cumulative_sum(a, None, 0, start=start)
            ctx.set_option("scan_onepass", 0)
            g0 = hip.cumulative_sum(a, None, 0, start=start)
        finally:
            ctx.set_option("scan_onepass", 1)
        assert g[0] == e[0] == STATUS_OK
        assert g[1].tobytes() == e[1].tobytes(), (n, "vs oracle")
        assert g[1].tobytes() == g2[1].tobytes() == g0[1].tobytes(), (n, "run to run / vs reduce-then-scan")


def test_cumulative_sum_one_pass_float64(hip, orc_be, ctx):
    """Round 6: Float64 columns without nulls take ONE pass too (scan_onepass_f64_kernel) — with a look-back whose GROUPING is fixed
    (tile totals → blocks of 64 tiles → super blocks of 4096, every tree a fixed 64-lane reduction), so the bytes are a function of the
    input alone: identical call after call, although which predecessor publishes first differs from launch to launch.
    (1) integer-valued data (every order exact): byte-equal to the sequential oracle and to reduce-then-scan (option scan_onepass 5);
    (2) general data: the tolerance of test_cumulative_sum_float — at most 64 + n/2^20 additions on the path to an output;
    (3) a running sum that overflows in a late tile stays ±inf / turns NaN like the sequential loop (vector_cumulative.go:228-318);
    sizes: around a tile (16 384 rows), more than one block (64 tiles), more tiles than resident workgroups, a start value."""
    rng = np.random.default_rng(606)
    tile = 1024 * 8 * 2
    for n in (1 << 18, (1 << 18) + 1, 17 * tile - 1, 17 * tile + 1, 70 * tile + 123, 300 * tile + 7, (1 << 23) + 5):
        xi = rng.integers(-3, 4, n).astype(np.float64)
        e = orc_be.cumulative_sum(xi, None, 0, start=np.float64(2))
        try:
            g = hip.cumulative_sum(xi, None, 0, start=np.float64(2))
            ctx.set_option("scan_onepass", 5)
            g0 = hip.cumulative_sum(xi, None, 0, start=np.float64(2))
        finally:
            ctx.set_option("scan_onepass", 1)
        assert g[0] == e[0] == STATUS_OK and g[1].tobytes() == e[1].tobytes() == g0[1].tobytes(), n
        x = rng.standard_normal(n) * 1e3
        runs = [hip.cumulative_sum(x, None, 0)[1] for _ in range(4)]
        assert all(r.tobytes() == runs[0].tobytes() for r in runs[1:]), (n, "run to run")
        exact = np.cumsum(x.astype(np.longdouble))
        mag = np.cumsum(np.abs(x.astype(np.longdouble)))
        tol = (n / 2**20 + 64) * 2.0**-53 * mag + 0.5 * 2.0**-52 * np.abs(exact)
        assert np.all(np.abs(runs[0].astype(np.longdouble) - exact) <= tol), n
    # overflow in a late tile, back in range right after (the tree alone would return to finite values), then the opposite infinity
    n = 90 * tile + 11
    big = np.float64(2.0 ** 1023)
    x = rng.integers(-4, 5, n).astype(np.float64)
    r = 77 * tile + 5
    x[r], x[r + 1], x[r + 2], x[r + 3] = big, big, -big, -big
    for edit in (None, (n - 2, -np.inf), ((r + n) // 2, np.nan)):
        y = x.copy()
        if edit:
            y[edit[0]] = edit[1]
        e, g = orc_be.cumulative_sum(y, None, 0)[1], hip.cumulative_sum(y, None, 0)[1]
        fin = np.isfinite(e)
        assert np.array_equal(fin, np.isfinite(g)) and g[fin].tobytes() == e[fin].tobytes()
        assert np.array_equal(np.isnan(e), np.isnan(g)) and np.array_equal(e[np.isinf(e)], g[np.isinf(g)])
        assert np.isfinite(e[r]) and not np.isfinite(e[r + 1])


@pytest.mark.parametrize("dtype", [np.int32, np.uint32, np.int64, np.uint64])
def test_cumulative_sum_one_pass_checked_and_nulls(hip, orc_be, ctx, dtype):
    """Round 5: the one-pass scan also takes CHECKED sums and columns WITH NULLS (4- / 8-byte integers): a null row adds nothing and
    keeps the zero of a fresh buffer, nulls skipped or not (then every row from the first null on is null: vector_cumulative.go:270-284);
    checked: "overflow" exactly when some running sum leaves the type's range (checkedAddSigned / Unsigned, :147-160) — decided from
    the wrapped prefixes by the step test (csrc/ah_scan.hip).  Byte-equal to the oracle and to reduce-then-scan (option scan_onepass 0),
    values and validity; overflow in the first tile, in a late tile and at the very last row; a running sum that touches the type's
    maximum exactly is NOT an overflow."""
    rng = np.random.default_rng(77)
    info = np.iinfo(dtype)
    tile = 1024 * 8 * (16 // np.dtype(dtype).itemsize)

    def both(a, valid, off, **kw):
        e = orc_be.cumulative_sum(a, valid, off, **kw)
        try:
            g = hip.cumulative_sum(a, valid, off, **kw)
            ctx.set_option("scan_onepass", 0)
            g0 = hip.cumulative_sum(a, valid, off, **kw)
        finally:
            ctx.set_option("scan_onepass", 1)
        assert g[0] == e[0] == g0[0], (kw, g[0], e[0], g0[0])
        if e[0] == STATUS_OK:
            n = a.size
            assert g[1].tobytes() == e[1].tobytes() == g0[1].tobytes(), kw
            if valid is not None:
                bits = lambda b: np.unpackbits(b, bitorder="little")[:n]
                assert (bits(g[2]) == bits(e[2])).all() and (bits(g0[2]) == bits(e[2])).all(), kw
                # whole bytes too: the last byte's bits from row n on are the pre-filled ones (prepareCumulativeOutput), not the kernel's
                assert g[2].tobytes() == e[2].tobytes() == g0[2].tobytes(), kw
            assert g[3] == e[3] == g0[3], kw
        return e[0]

    small = max(int(info.max // (1 << 27)), 1)     # 2^24 rows of at most `small` cannot leave the range
    for n in ((1 << 18) + 3, 17 * tile + 1, 70 * tile + 123, (1 << 23) + 5):
        a = rng.integers(-small if info.min < 0 else 0, small, n, dtype=dtype, endpoint=True)
        valid = rand_bits(rng, n + 16, 0.9)
        start = dtype(rng.integers(0, small, dtype=dtype))
        for off in (0, 5):
            assert both(a, valid, off, start=start, skip_nulls=True, checked=False) == STATUS_OK
            assert both(a, valid, off, start=start, skip_nulls=True, checked=True) == STATUS_OK
        late = valid.copy()
        late[: (n // 2) // 8] = 0xFF                       # no null in the first half: the first null lies in a late tile
        assert both(a, late, 0, start=start, skip_nulls=False, checked=True) == STATUS_OK
        assert both(a, valid, 3, skip_nulls=False, checked=False) == STATUS_OK
        assert both(a, None, 0, start=start, checked=True) == STATUS_OK
        # wrap-around (unchecked) with nulls: full-range values
        wide = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
        assert both(wide, valid, 0, skip_nulls=True, checked=False) == STATUS_OK
        assert both(wide, None, 0, checked=True) == STATUS_EOVERFLOW
        # exactly one step leaves the range, at a chosen row; everything before it stays far inside
        for where in (5, n // 2 + 11, n - 1):
            z = np.zeros(n, dtype=dtype)
            z[0] = info.max - 10
            z[where] = 10                                    # the running sum touches the maximum: no overflow
            assert both(z, None, 0, checked=True) == STATUS_OK
            z[where] = 11                                    # one beyond
            assert both(z, None, 0, checked=True) == STATUS_EOVERFLOW
            v = np.full((n + 7) // 8 + 8, 0xFF, np.uint8)
            v[where // 8] &= ~np.uint8(1 << (where % 8))     # … unless that row is null
            assert both(z, v, 0, skip_nulls=True, checked=True) == STATUS_OK
            if info.min < 0:
                z[0] = info.min + 10
                z[where] = -11
                assert both(z, None, 0, checked=True) == STATUS_EOVERFLOW
                z[where] = -10
                assert both(z, None, 0, checked=True) == STATUS_OK


def test_hash_sum_quick_look_on_a_periodic_column(hip, orc_be, ctx):
    """A column built by tiling one block (period 2^16 rows, 40 000 keys) — what benchmarks do.  An equidistant sample whose stride
    divides the period reads the same 128 rows over and over and takes 40 000 groups for 128: the direct path was chosen, its global
    table filled up and every further row walked all of it (0.9 s for 2^26 rows).  The quick look's sample positions are jittered
    inside their strides, and a voided attempt stops feeding its tables; the result is the oracle's either way."""
    import time
    rng = np.random.default_rng(404)
    block = (rng.integers(0, 40_000, 1 << 16).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
    n = 1 << 23
    keys = np.tile(block, n >> 16)
    vals = rng.integers(-1000, 1000, n).astype(np.float64)
    g = hip.hash_sum("f64", keys, None, 0, vals, None, 0)
    e = orc_be.hash_sum("f64", keys, None, 0, vals, None, 0)
    for i in (0, 1, 2, 4):
        assert g[i].tobytes() == e[i].tobytes(), i
    # … and it must not fall off a cliff: device-resident, a second call, generously bounded (the cliff was 100 ms at this size)
    dk, dv = ctx.to_device(keys), ctx.to_device(vals)
    outs = [ctx.alloc((n + 1) * 8 + 64) for _ in range(4)]
    ctx.hash_sum("f64", dk, None, 0, dv, None, 0, n, *outs)
    ctx.sync()
    t0 = time.perf_counter()
    ctx.hash_sum("f64", dk, None, 0, dv, None, 0, n, *outs)
    ctx.sync()
    assert time.perf_counter() - t0 < 0.02, time.perf_counter() - t0


@pytest.mark.parametrize("case", ["ordinary", "outlier_missed_by_the_sample", "outlier_within_the_margin", "wide_but_fits", "too_wide"])
def test_hash_sum_f64_scale_from_sample(hip, orc_be, ctx, case):
    """The no-cut group-by (≤ 2048 groups, ≥ 2^22 rows) takes its fixed-point scale from 2^18 sampled values + 4 binades and lets the
    aggregate pass verify it (csrc/ah_groupby.hip, fx_guess_check_kernel).  Whatever the sample saw, the sums must be the exact
    per-group sums, correctly rounded — with the guess, with the full absmax pass (option groupby_scale_guess 0) and run to run:
    an outlier the sample cannot see (handed to the id-based path), one inside the margin, a column 36 binades wide (fits the guess),
    one 60 binades wide (handed over)."""
    import math
    from fractions import Fraction
    rng = np.random.default_rng(912)
    n = (1 << 22) + 777
    keys = rng.integers(0, 900, n).astype(np.int64) * 1000003
    fv = rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)      # one binade, so that the cases below control the range
    fv[rng.integers(0, n, 50)] = 0.0
    lone = 64 * 12345 + 17          # the sample reads rows 0 … 63 of every (n / 4096 rounded down to 64)-row stride: this row is never in it
    stride = (n // 4096) & ~63
    assert lone % stride >= 64
    if case == "outlier_missed_by_the_sample":
        fv[lone] = 3.0e9            # 2^31: beyond the margin (4) + the accumulator's slack (2)
    elif case == "outlier_within_the_margin":
        fv[lone] = 40.0             # 2^5 above the sampled maximum's binade
    elif case == "wide_but_fits":
        fv[rng.integers(0, n, 2000)] *= 2.0 ** -36   # guess = sampled exponent + 4: 40 binades to cover, 42 allowed
    elif case == "too_wide":
        fv[rng.integers(0, n, 2000)] *= 2.0 ** -60
    vvalid = rand_bits(rng, n + 8, 0.9)
    ok = np.unpackbits(vvalid, bitorder="little")[3:3 + n].astype(bool)
    ok[lone] = True
    vvalid = np.packbits(np.concatenate([np.ones(3, bool), ok, np.ones(8, bool)]), bitorder="little")
    res = {}
    try:
        for guess in (1, 0):
            ctx.set_option("groupby_scale_guess", guess)
            res[guess] = hip.hash_sum("f64", keys, None, 0, fv, vvalid, 3)
        ctx.set_option("groupby_scale_guess", 1)
        again = hip.hash_sum("f64", keys, None, 0, fv, vvalid, 3)
    finally:
        ctx.set_option("groupby_scale_guess", 1)
    e = orc_be.hash_sum("f64", keys, None, 0, fv, vvalid, 3)
    g = res[1]
    assert g[0].tobytes() == e[0].tobytes() and g[2].tobytes() == e[2].tobytes()
    assert g[1].tobytes() == again[1].tobytes()
    if case != "too_wide":          # one scale for the call, no addend truncated: both ways are the correctly rounded exact sums
        assert g[1].tobytes() == res[0][1].tobytes()
    pos = {int(k): i for i, k in enumerate(g[0].view(np.int64))}
    for k, (exact, cnt, gmax) in _exact_group_sums(keys, fv, ok, 900).items():
        got = float(g[1][pos[k]])
        if case == "too_wide":      # per-group scales: the documented bound
            assert abs(Fraction(got) - exact) <= Fraction(0.5 * math.ulp(got)) + Fraction(gmax) * cnt / 2**93, (case, k, got, float(exact))
        else:
            assert abs(Fraction(got) - exact) <= Fraction(0.5 * math.ulp(got)), (case, k, got, float(exact))


# ---- fused ---------------------------------------------------------------------------------
def test_fused_vs_unfused_chain(hip, orc_be):
    rng = np.random.default_rng(81)
    for n in [1, 2, 3, 1023, 2049, 70001, 1 << 20]:
        x = rng.integers(-2**62, 2**62, n, dtype=np.int64)
        valid = rand_bits(rng, n + 16, 0.9)
        thr = int(np.percentile(x, 50)) if n > 2 else 0
        for cmpop in (EQ, NE, GT, GE):
            for off, v in [(0, None), (0, valid), (5, valid)]:
                for mis in (0, 1):
                    assert hip.cmp_filter_sum_i64(cmpop, x, v, off, thr, mis) == orc_be.cmp_filter_sum_i64(cmpop, x, v, off, thr)
        xf = rng.uniform(-1, 1, n)
        for off, v in [(0, None), (3, valid)]:
            s, c = hip.cmp_filter_sum_f64(GT, xf, v, off, 0.1)
            es, ec = orc_be.cmp_filter_sum_f64(GT, xf, v, off, 0.1)
            assert c == ec and abs(s - es) <= math.ulp(es) if es != 0 else s == 0


def test_fused_equals_separate_gpu_kernels(hip, ctx):
    """Compare → Filter → Sum run as three GPU calls must equal the fused call."""
    rng = np.random.default_rng(82)
    n = 200003
    x = rng.integers(-10**6, 10**6, n, dtype=np.int64)
    thr = 1234
    mask = hip.comparison(GT, AS, x, np.array([thr], np.int64), np.zeros(n // 8 + 8, np.uint8))
    kept, _, _ = hip.filter(x, None, 0, mask, None, 0, n, DROP, False)
    assert (hip.sum(kept), len(kept)) == hip.cmp_filter_sum_i64(GT, x, None, 0, thr)


# ---- cumulative_sum ------------------------------------------------------------------------
CUMSUM_SIZES = [1, 2, 3, 15, 17, 63, 65, 255, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 8191, 8192, 8193, 16385, 70001, 300007, 1200011]


def cumsum_valid_equal(got, exp, n):
    """only bits [0, n) belong to the result; the reference pre-fills whole bytes with ones"""
    return bool(np.array_equal(OL.unpack_bits(got, 0, n), OL.unpack_bits(exp, 0, n)))


@pytest.mark.parametrize("dtype", OL.INT_DTYPES, ids=str)
def test_cumulative_sum_int_bit_exact(hip, orc_be, dtype):
    """Unchecked integer running sums wrap exactly like Go's `current += v`; bit-exact for every
    width, with / without nulls, both null modes, sliced validity, misaligned values, a start value."""
    rng = np.random.default_rng(1000 + np.dtype(dtype).itemsize)
    for k, n in enumerate(CUMSUM_SIZES):
        x = rand(rng, dtype, n)
        start = None if k % 3 == 0 else x.dtype.type(rng.integers(0, 100))
        mis = k % 4
        st_e, e, _, _ = orc_be.cumulative_sum(x, None, 0, start, False, False)
        st_g, g, _, _ = hip.cumulative_sum(x, None, 0, start, False, False, misalign=mis)
        assert st_e == st_g == STATUS_OK and g.tobytes() == e.tobytes(), (dtype, n)
        off = int(rng.integers(0, 70))
        for p_null, skip in ((0.3, True), (0.3, False), (2.0 / max(n, 1), False), (0.999, True)):
            bits = OL.pack_bits([True] * off + list(rng.random(n) >= p_null))
            st_e, e, ev, en = orc_be.cumulative_sum(x, bits, off, start, skip, False)
            st_g, g, gv, gn = hip.cumulative_sum(x, bits, off, start, skip, False, misalign=mis)
            assert st_e == st_g == STATUS_OK
            assert g.tobytes() == e.tobytes(), (dtype, n, p_null, skip)
            assert cumsum_valid_equal(gv, ev, n) and gn == en, (dtype, n, p_null, skip)


@pytest.mark.parametrize("dtype", OL.INT_DTYPES, ids=str)
def test_cumulative_sum_checked_parity(hip, orc_be, dtype):
    """checked: same values when no running sum leaves the range, "overflow" exactly when one does —
    including sums that leave the range and return, and overflows only reachable through null rows."""
    rng = np.random.default_rng(2000 + np.dtype(dtype).itemsize)
    info = np.iinfo(dtype)
    n_over = 0
    for n in (5, 64, 257, 1024, 2049, 9000, 70001):
        for trial in range(6):
            # steps sized so that roughly half the trials overflow somewhere
            amp = max(1, int(1.5 * info.max / math.sqrt(n))) if trial % 2 == 0 else max(1, int(info.max // (4 * n)))
            lo = -amp if info.min < 0 else 0
            x = rng.integers(lo, min(amp, int(info.max)), n, endpoint=True, dtype=dtype)
            bits = None if trial < 2 else OL.pack_bits(list(rng.random(n) >= 0.1))
            skip = trial % 3 != 0
            st_e, e, ev, en = orc_be.cumulative_sum(x, bits, 0, None, skip, True)
            st_g, g, gv, gn = hip.cumulative_sum(x, bits, 0, None, skip, True)
            assert st_e == st_g, (dtype, n, trial, st_e, st_g)
            n_over += st_e != STATUS_OK
            if st_e == STATUS_OK:
                assert g.tobytes() == e.tobytes()
                if bits is not None:
                    assert cumsum_valid_equal(gv, ev, n) and gn == en
    assert n_over > 0
    # a single out-of-range running sum in the middle of a long column, then back in range
    n = 500000
    x = np.zeros(n, dtype)
    x[1234] = info.max; x[300000] = 1; x[300001] = np.array(-1 if info.min < 0 else 0).astype(dtype)
    assert hip.cumulative_sum(x, None, 0, None, False, True)[0] == orc_be.cumulative_sum(x, None, 0, None, False, True)[0] != STATUS_OK
    x[300000] = 0
    st_g, g, _, _ = hip.cumulative_sum(x, None, 0, None, False, True)
    st_e, e, _, _ = orc_be.cumulative_sum(x, None, 0, None, False, True)
    assert st_g == st_e == STATUS_OK and g.tobytes() == e.tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=str)
def test_cumulative_sum_float(hip, orc_be, dtype):
    """Floats: the reference adds sequentially in T; the scan adds in float64 along a fixed tree
    (element → 16-byte vector → 64-lane wave scan → ≤ 8 vectors → 4 waves → ≤ 7 tiles → super-tile
    scan): at most 64 + n/2^20 additions lie on the path to any output, and the result is a pure
    function of the data (no timing dependence).
    (1) integer-valued data whose sums stay below 2^24 / 2^53: every order is exact → bit-exact.
    (2) general data, tolerance stated here and in DESIGN.md §4: with E = the exact prefix sums,
        |gpu − E| ≤ (64 + n/2^20)·2^-53·Σ_{j≤i}|x_j|  (+ ½ulp_T(E) for the final rounding to T);
        the reference's own bound for the same data is (i+1)·eps_T·Σ|x| — ours is the tighter one."""
    rng = np.random.default_rng(3000 + np.dtype(dtype).itemsize)
    eps_t = float(np.finfo(dtype).eps)
    for k, n in enumerate(CUMSUM_SIZES):
        xi = rng.integers(-3, 4, n).astype(dtype)
        bits = OL.pack_bits(list(rng.random(n) >= 0.2)) if k % 2 else None
        st_e, e, ev, en = orc_be.cumulative_sum(xi, bits, 0, dtype(2), True, False)
        st_g, g, gv, gn = hip.cumulative_sum(xi, bits, 0, dtype(2), True, False, misalign=k % 3)
        assert st_e == st_g == STATUS_OK and g.tobytes() == e.tobytes(), (dtype, n)
        if bits is not None:
            assert cumsum_valid_equal(gv, ev, n) and gn == en
        x = (rng.standard_normal(n) * 1e3).astype(dtype)
        st_g, g, _, _ = hip.cumulative_sum(x, None, 0, None, False, False)
        st_e, e, _, _ = orc_be.cumulative_sum(x, None, 0, None, False, False)
        exact = np.cumsum(x.astype(np.longdouble))
        mag = np.cumsum(np.abs(x.astype(np.longdouble)))
        tol = (n / 2**20 + 64) * 2.0**-53 * mag + 0.5 * eps_t * np.abs(exact)
        assert np.all(np.abs(g.astype(np.longdouble) - exact) <= tol), (dtype, n)
        # and the oracle (the reference's order) sits inside ITS bound around the same exact values
        assert np.all(np.abs(e.astype(np.longdouble) - exact) <= (np.arange(n) + 1) * eps_t * mag)
    # non-finite values propagate like the sequential loop: from the first NaN/inf on
    x = np.ones(5000, dtype); x[4000] = np.inf; x[4500] = -np.inf
    g = hip.cumulative_sum(x, None, 0, None, False, False)[1]
    e = orc_be.cumulative_sum(x, None, 0, None, False, False)[1]
    assert np.array_equal(g[:4500], e[:4500]) and np.all(np.isnan(g[4500:])) and np.all(np.isnan(e[4500:]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cumulative_sum_float_overflow_sticks(ctx, hip, orc_be, dtype):
    """a running sum that reaches ±inf STAYS there in the reference's sequential loop (vector_cumulative.go:228-318), whatever
    finite values follow; the opposite infinity or a NaN turns it into NaN for good.  The tree scan alone would come back to
    finite values — the first non-finite row is found by the scan and the sequential state is forced from there on.
    Values are powers of two so that every finite prefix is exact in any order: the comparison with the oracle is bit for
    bit on the finite rows and class for class (±inf / NaN) on the rest."""
    big = dtype(2.0 ** (127 if dtype == np.float32 else 1023))
    rng = np.random.default_rng(7)

    def check(x, bits=None, skip=True):
        st_e, e, ev, en = orc_be.cumulative_sum(x, bits, 0, None, skip, False)
        st_g, g, gv, gn = hip.cumulative_sum(x, bits, 0, None, skip, False)
        assert st_e == st_g == STATUS_OK
        fin = np.isfinite(e)
        assert np.array_equal(fin, np.isfinite(g))
        assert g[fin].tobytes() == e[fin].tobytes()
        assert np.array_equal(np.isnan(e), np.isnan(g)) and np.array_equal(e[np.isinf(e)], g[np.isinf(g)])
        if bits is not None:
            assert cumsum_valid_equal(gv, ev, x.size) and gn == en
        return e

    for n in (10, 5000, 70001, (1 << 21) + 17):
        x = rng.integers(-4, 5, n).astype(dtype)
        r = n // 3
        x[r], x[r + 1] = big, big                       # overflow to +inf at r + 1 …
        x[r + 2], x[r + 3] = -big, -big                 # … the true sum is back in range right after
        e = check(x)
        assert np.isfinite(e[r]) and np.all(e[r + 1:] == np.inf)
        y = x.copy(); y[n - 2] = -np.inf                # the opposite infinity: NaN from there on
        e = check(y)
        assert np.all(e[r + 1:n - 2] == np.inf) and np.all(np.isnan(e[n - 2:]))
        y = -x; y[(r + n) // 2] = np.nan                # −inf, then a NaN addend
        e = check(y)
        assert np.all(e[r + 1:(r + n) // 2] == -np.inf) and np.all(np.isnan(e[(r + n) // 2:]))
        keep = rng.random(n) >= 0.2
        keep[r:r + 4] = True                             # (with x[r] or x[r + 1] null no prefix overflows, but −big − big would overflow
        bits = OL.pack_bits(list(keep))                  #  inside one 16-byte vector of the tree: the corner DESIGN.md §4 documents)
        # nulls: skipped rows keep payload 0 and do not disturb the state
        check(x, bits, True)
        check(y, bits, True)
        check(x, bits, False)
    # several segments (the running total crosses them through device memory): forced small here
    ctx.set_option("scan_segment_log2", 16)
    try:
        n = 300_007
        x = rng.integers(-4, 5, n).astype(dtype); x[1000], x[1001] = big, big; x[250_000] = -np.inf
        check(x)
        xi = rng.integers(-1000, 1000, n).astype(np.int64)
        assert hip.cumulative_sum(xi, None, 0)[1].tobytes() == orc_be.cumulative_sum(xi, None, 0)[1].tobytes()
        bits = OL.pack_bits(list(rng.random(n) >= 0.1))
        for skip in (True, False):
            g, e = hip.cumulative_sum(xi, bits, 0, None, skip, True), orc_be.cumulative_sum(xi, bits, 0, None, skip, True)
            assert g[0] == e[0] == STATUS_OK and g[1].tobytes() == e[1].tobytes() and g[3] == e[3]
    finally:
        ctx.set_option("scan_segment_log2", 0)


def test_cumulative_sum_many_tiles(hip, orc_be):
    """many tiles and super tiles (2^24 rows): tile sums → super-tile prefix → in-tile scan; and the
    result does not change from run to run (also for floats: the summation tree is fixed)"""
    rng = np.random.default_rng(77)
    for dtype, n in ((np.int64, (1 << 24) + 3), (np.int8, (1 << 24) + 5), (np.uint32, (1 << 23) + 1)):
        x = rand(rng, dtype, n)
        e = orc_be.cumulative_sum(x, None, 0, None, False, False)[1]
        for rep in range(2):
            g = hip.cumulative_sum(x, None, 0, None, False, False)[1]
            assert g.tobytes() == e.tobytes(), (dtype, rep)
    xf = (rng.standard_normal((1 << 23) + 7) * 1e3)
    runs = [hip.cumulative_sum(xf, None, 0, None, False, False)[1].tobytes() for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


# ---- numeric cast --------------------------------------------------------------------------
CAST_SIZES = [1, 3, 15, 17, 63, 65, 1023, 1025, 4097, 16385, 70001, 300007]


def cast_input(rng, frm, to, n, in_range):
    fd, td = np.dtype(frm), np.dtype(to)
    if fd.kind == "f" and td.kind != "f":
        if in_range:
            info = np.iinfo(td)
            a = np.trunc(rng.uniform(max(float(info.min), -2.0**52), min(float(info.max), 2.0**52), n)).astype(fd)
            hi = fd.type(float(info.max)) if float(fd.type(float(info.max))) <= float(info.max) else np.nextafter(fd.type(float(info.max)), fd.type(0))
            return np.clip(a, fd.type(float(info.min)), hi)
        a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 25, n)).astype(fd)
        if n > 8:
            a[rng.integers(0, n, 4)] = [np.nan, np.inf, -np.inf, -0.0]
        return a
    if fd.kind != "f" and in_range:  # values every target can hold
        return rng.integers(0, 100, n).astype(fd)
    return rand(rng, frm, n)


@pytest.mark.parametrize("frm", OL.ALL_DTYPES, ids=str)
def test_cast_unchecked_bit_exact(hip, orc_be, frm):
    """allow_int_overflow + allow_float_truncate: every slot converted, bit-exact against the oracle for
    all 9 targets — wraparound, sign extension, round-to-nearest-even int → float and f64 → f32, and the
    stated float → int rule (truncate into 64 bits saturating, NaN → 0, keep the low bits)."""
    rng = np.random.default_rng(4000 + OL.TYPE_IDS[np.dtype(frm)])
    for to in OL.ALL_DTYPES:
        if to == frm:
            continue
        for k, n in enumerate(CAST_SIZES):
            a = cast_input(rng, frm, to, n, in_range=False)
            st_e, e, _ = orc_be.cast_numeric(a, to, None, 0, True, True)
            st_g, g, _ = hip.cast_numeric(a, to, None, 0, True, True, misalign=k % 3)
            assert st_e == st_g == STATUS_OK
            assert same_bits_or_both_nan(g, e), (frm, to, n)


@pytest.mark.parametrize("frm", OL.ALL_DTYPES, ids=str)
def test_cast_safe_parity(hip, orc_be, frm):
    """safe casts: same values when nothing fails; the same FIRST offender and the reference's message
    when something does; offenders under null slots never fail."""
    rng = np.random.default_rng(5000 + OL.TYPE_IDS[np.dtype(frm)])
    n_fail = 0
    for to in OL.ALL_DTYPES:
        if to == frm:
            continue
        for k, n in enumerate(CAST_SIZES):
            ok_in = cast_input(rng, frm, to, n, in_range=True)
            st_e, e, _ = orc_be.cast_numeric(ok_in, to)
            st_g, g, _ = hip.cast_numeric(ok_in, to, misalign=k % 2)
            assert st_e == st_g == STATUS_OK, (frm, to, n)
            assert g.tobytes() == e.tobytes(), (frm, to, n)
            # now with offenders: under nulls → still fine; one valid offender → the same error text
            bad_in = cast_input(rng, frm, to, n, in_range=False)
            off = int(rng.integers(0, 9))
            st_all, _, msg_all = orc_be.cast_numeric(bad_in, to)
            if st_all == STATUS_OK:
                continue
            # find the offending rows through the oracle: null them all → success
            flags = np.ones(n, bool)
            pos = []
            while True:
                bits = OL.pack_bits([True] * off + flags.tolist())
                st_e, e, msg = orc_be.cast_numeric(bad_in, to, bits, off)
                if st_e == STATUS_OK or len(pos) > 3:
                    break
                # the message names the value; mask the first row holding an offender by bisection on prefixes
                lo_, hi_ = 0, n
                while hi_ - lo_ > 1:
                    mid = (lo_ + hi_) // 2
                    f2 = flags.copy(); f2[mid:] = False
                    st_m, _, _ = orc_be.cast_numeric(bad_in, to, OL.pack_bits([True] * off + f2.tolist()), off)
                    if st_m == STATUS_OK:
                        lo_ = mid
                    else:
                        hi_ = mid
                pos.append(lo_)
                st_g, g, msg_g = hip.cast_numeric(bad_in, to, bits, off)
                assert st_g == STATUS_EINVALID and msg_g.endswith(msg), (frm, to, n, msg_g, msg)
                n_fail += 1
                flags[lo_] = False
            if st_e == STATUS_OK:
                st_g, g, _ = hip.cast_numeric(bad_in, to, bits, off)
                assert st_g == STATUS_OK and same_bits_or_both_nan(g, e), (frm, to, n)
    assert n_fail > 0


def test_cast_bool_to_numeric_random(hip, orc_be):
    rng = np.random.default_rng(6000)
    for n in (1, 7, 64, 65, 1000, 70001):
        off = int(rng.integers(0, 70))
        bits = OL.pack_bits(list(rng.random(off + n) < 0.5))
        for dt in OL.ALL_DTYPES:
            assert hip.cast_bool_to_numeric(bits, off, n, dt).tobytes() == orc_be.cast_bool_to_numeric(bits, off, n, dt).tobytes()


# ---- is_in -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32, np.float32, np.int64, np.uint64, np.float64], ids=str)
def test_is_in_random(hip, orc_be, dtype):
    """bitmap path (1/2-byte keys), LDS table (small sets), HBM table (large sets): data and validity
    bitmaps bit-exact for all four null behaviours, sliced validity on both sides, output at a bit offset."""
    rng = np.random.default_rng(7000 + OL.TYPE_IDS[np.dtype(dtype)])
    dt = np.dtype(dtype)
    for n in (1, 63, 64, 65, 1000, 4097, 70001):
        for set_n in (0, 1, 7, 300, 2500, 5000):   # LDS table · 128 KiB LDS table (1025 … 4096 keys) · HBM table
            universe = max(4, 3 * set_n)
            def draw(m):
                if dt.kind == "f":
                    return rng.integers(0, universe, m).astype(dt)
                return rng.integers(0, min(universe, int(np.iinfo(dt).max)), m).astype(dt)
            vals, vset = draw(n), draw(set_n)
            if dt.itemsize == 8 and set_n > 1:
                vset[0] = np.array([2**64 - 1], np.uint64).view(dt)[0]; vals[n // 2] = vset[0]   # the all-ones key
            off, soff = int(rng.integers(0, 20)), int(rng.integers(0, 20))
            valid = OL.pack_bits([True] * off + list(rng.random(n) >= 0.2)) if n % 2 else None
            svalid = OL.pack_bits([True] * soff + list(rng.random(set_n) >= 0.3)) if set_n % 2 else None
            for nb in (0, 1, 2, 3):
                out_off = int(rng.integers(0, 70)) if nb % 2 else 0
                fill = 0xFF if nb == 3 else 0
                ed, ev = orc_be.is_in(vals, valid, off, vset, svalid, soff, nb, out_off, fill)
                gd, gv = hip.is_in(vals, valid, off, vset, svalid, soff, nb, out_off, fill, misalign=n % 3)
                assert gd.tobytes() == ed.tobytes() and gv.tobytes() == ev.tobytes(), (dtype, n, set_n, nb, out_off)


def test_is_in_large_set(hip, orc_be):
    rng = np.random.default_rng(7100)
    vset = rng.integers(-2**62, 2**62, 200003, dtype=np.int64)
    vals = np.concatenate([rng.choice(vset, 150000), rng.integers(-2**62, 2**62, 150001, dtype=np.int64)])
    rng.shuffle(vals)
    ed, ev = orc_be.is_in(vals, None, 0, vset, None, 0, 0)
    gd, gv = hip.is_in(vals, None, 0, vset, None, 0, 0)
    assert gd.tobytes() == ed.tobytes() and gv.tobytes() == ev.tobytes()
    assert 140000 < int(np.unpackbits(gd, bitorder="little")[:vals.size].sum()) < 160000


# ---- sort_indices ----------------------------------------------------------------------------
SORT_SIZES = [1, 2, 63, 64, 65, 511, 2047, 2048, 2049, 4097, 70001, 300007]


@pytest.mark.parametrize("dtype", OL.ALL_DTYPES, ids=str)
def test_sort_indices_bit_exact(hip, orc_be, dtype):
    """the permutation itself is compared (a stable sort has exactly one answer): heavy duplicates,
    full-range values, nulls, NaN / ±inf / ±0, both orders and both null placements, sliced validity"""
    rng = np.random.default_rng(8000 + OL.TYPE_IDS[np.dtype(dtype)])
    dt = np.dtype(dtype)
    for k, n in enumerate(SORT_SIZES):
        for flavour in range(3):
            if flavour == 0:      # few distinct values: ties everywhere
                a = rng.integers(0, 7, n).astype(dt)
            elif flavour == 1:    # full range
                a = rand(rng, dtype, n)
            else:                 # small range around zero, negative where the type allows
                a = (rng.integers(0, 2000, n) - (1000 if dt.kind != "u" else 0)).astype(dt)
            if dt.kind == "f" and n > 16:
                a[rng.integers(0, n, 6)] = [np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0]
            off = int(rng.integers(0, 40))
            valid = OL.pack_bits([True] * off + list(rng.random(n) >= 0.15)) if (k + flavour) % 2 else None
            desc, at_start = bool((k + flavour) & 1), bool((k >> 1) & 1)
            e = orc_be.sort_indices(a, valid, off, desc, at_start)
            g = hip.sort_indices(a, valid, off, desc, at_start, misalign=k % 3)
            assert g.tobytes() == e.tobytes(), (dtype, n, flavour, desc, at_start)


def test_sort_indices_many_tiles(hip, orc_be):
    rng = np.random.default_rng(8100)
    n = (1 << 22) + 77
    for dtype in (np.int64, np.float64, np.uint16):
        a = rand(rng, dtype, n) if dtype != np.uint16 else rng.integers(0, 65536, n).astype(np.uint16)
        valid = OL.pack_bits(list(rng.random(n) >= 0.05))
        e = orc_be.sort_indices(a, valid, 0, False, False)
        g = hip.sort_indices(a, valid, 0, False, False)
        assert g.tobytes() == e.tobytes(), dtype
    # already sorted / reverse sorted / constant columns
    for a in (np.arange(n, dtype=np.int64), np.arange(n, 0, -1, dtype=np.int64), np.full(n, 42, np.int64)):
        assert hip.sort_indices(a, None, 0, True, False).tobytes() == orc_be.sort_indices(a, None, 0, True, False).tobytes()


def test_sort_indices_msd_path(ctx, hip, orc_be):
    """≥ 2^22 rows with ≥ 4 varying key bytes take ah_sort_msd.hip (bucket map from a sample → two MSD partition passes → one
    wave per bucket on (key, row)); columns it cannot balance fall back to the LSD passes.  Either way the permutation is the
    oracle's, and the same as with the path switched off."""
    rng = np.random.default_rng(8300)
    n = (1 << 22) + 12345
    cases = {
        "int64 full range": rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64),
        "uint64": rng.integers(0, 2**64 - 1, n, dtype=np.uint64),
        "float64 normal": rng.standard_normal(n),
        "float64 lognormal": np.exp(rng.standard_normal(n) * 8),
        "float64 uniform(-1, 1)": rng.uniform(-1, 1, n),
        "int64 clustered": 10**15 + rng.integers(0, 10**11, n),
        "int64 two clusters": np.where(rng.random(n) < 0.3, rng.integers(0, 10**6, n), 2**60 + rng.integers(0, 2**40, n)),
        "int64 ties among wide keys": rng.integers(0, 2**40, n // 4, dtype=np.int64)[rng.integers(0, n // 4, n)] * 1000003,
        "float32": (rng.standard_normal(n) * 1e3).astype(np.float32),
        "int64 dense, ties inside the buckets": rng.integers(0, 2**27, n, dtype=np.int64),          # one-word elements carrying the row
        "int64 wide, a few equal pairs": np.concatenate([w := rng.integers(-2**62, 2**62, n - 5000, dtype=np.int64), w[:5000]])[rng.permutation(n)],
        "int64 heavy duplicates (falls back)": rng.integers(0, 2**50, 3000, dtype=np.int64)[rng.integers(0, 3000, n)],
        "int64 one hot key (falls back)": np.where(rng.random(n) < 0.2, np.int64(123456789012345), rng.integers(-2**62, 2**62, n, dtype=np.int64)),
    }
    # a second length, one row past a tile boundary (n itself ends 57 rows into a tile), with constant high bits: only the low 40 bits
    # vary, so the bucket map works on shifted keys.  (The map is built from sample quantiles: it fills every level-1 parent
    # whatever the keys are — a parent without rows is reached through the two-cut encode and group-by, whose parents are hash bits.)
    cases["int64 constant high bits, a tile and one row more"] = (np.int64(0x5A) << 56) + rng.integers(0, 2**40, (1 << 22) + 4097, dtype=np.int64)
    for name, a in cases.items():
        a = np.ascontiguousarray(a)
        n = a.size
        if a.dtype.kind == "f":
            a[rng.integers(0, n, 6)] = [np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0]
        valid = OL.pack_bits(list(rng.random(n + 9) >= 0.03))
        for desc, at_start, v, off in [(False, False, valid, 9), (True, True, None, 0)]:
            e = orc_be.sort_indices(a, v, off, desc, at_start)
            g = hip.sort_indices(a, v, off, desc, at_start)
            assert g.tobytes() == e.tobytes(), (name, desc)
        try:
            ctx.set_option("sort_msd", 0)
            g0 = hip.sort_indices(a, None, 0, False, False)
        finally:
            ctx.set_option("sort_msd", 1)
        assert g0.tobytes() == hip.sort_indices(a, None, 0, False, False).tobytes(), name


def test_sort_indices_multi_key(hip, orc_be):
    """record-batch sort: 1–4 keys of mixed types, orders and null placements, few distinct values per key
    so that later keys decide most positions; the permutation must equal the oracle's exactly"""
    rng = np.random.default_rng(8200)
    dts = [np.int8, np.uint16, np.int32, np.float32, np.int64, np.float64, np.uint64]
    for n in (1, 65, 2049, 70001):
        for trial in range(6):
            nk = 1 + trial % 4
            cols = []
            for k in range(nk):
                dt = np.dtype(dts[int(rng.integers(0, len(dts)))])
                a = rng.integers(0, 4 if k < nk - 1 else 50, n).astype(dt)
                if dt.kind == "f" and n > 8:
                    a[rng.integers(0, n, 3)] = np.nan
                valid = OL.pack_bits(list(rng.random(n) >= 0.1)) if rng.random() < 0.6 else None
                cols.append((a, valid, 0, bool(rng.integers(0, 2)), bool(rng.integers(0, 2))))
            e = orc_be.sort_indices_multi(cols)
            g = hip.sort_indices_multi(cols)
            assert g.tobytes() == e.tobytes(), (n, trial, [(c[0].dtype, c[3], c[4]) for c in cols])


def test_take_boolean_bit_exact(ctx, orc):
    rng = np.random.default_rng(9200)
    for nvals in (1, 70, 5000):
        voff = int(rng.integers(0, 20))
        data = OL.pack_bits(list(rng.random(nvals + voff) < 0.5)); vvalid = OL.pack_bits(list(rng.random(nvals + voff) >= 0.2))
        db = ctx.to_device(np.concatenate([data, np.zeros(8, np.uint8)])); vb = ctx.to_device(np.concatenate([vvalid, np.zeros(8, np.uint8)]))
        for n, idt in ((1, np.int8), (64, np.uint8), (1000, np.int16), (70001, np.int32), (999, np.uint64)):
            idx = rng.integers(0, min(nvals, np.iinfo(idt).max + 1), n).astype(idt)
            ivalid = OL.pack_bits(list(rng.random(n) >= 0.1))
            ib = ctx.to_device(idx); ivb = ctx.to_device(np.concatenate([ivalid, np.zeros(8, np.uint8)]))
            od = ctx.alloc((n + 7) // 8 + 64); ov = ctx.alloc((n + 7) // 8 + 64)
            nulls = ctx.take_boolean(db, vb, voff, nvals, idx.dtype.itemsize, idx.dtype.kind == "i", ib, ivb, 0, n, od, ov)
            st, ed, ev, en, _ = orc.take_boolean(data, vvalid, voff, nvals, idx, ivalid, 0, True)
            nb = (n + 7) // 8
            assert st == 0 and nulls == en
            assert od.download(np.uint8, nb).tobytes() == ed.tobytes() and ov.download(np.uint8, nb).tobytes() == ev.tobytes(), (nvals, n, idt)


# ---- var-length take / filter -----------------------------------------------------------------
def random_binary(rng, n, odt, mean_len, p_null):
    lens = rng.geometric(1.0 / (mean_len + 1), n) - 1
    lens[rng.random(n) < 0.1] = 0
    offsets = np.zeros(n + 1, odt)
    offsets[1:] = np.cumsum(lens)
    data = rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    valid = OL.pack_bits(list(rng.random(n) >= p_null)) if p_null > 0 else None
    return offsets, data, valid


@pytest.mark.parametrize("odt", [np.int32, np.int64], ids=["binary", "large_binary"])
def test_take_binary_bit_exact(hip, orc_be, odt):
    """offsets, data bytes, validity and null count all byte-identical; short and long values, repeats,
    nulls on both sides, every index width, sliced values"""
    rng = np.random.default_rng(9000 + np.dtype(odt).itemsize)
    for nvals, mean_len in ((1, 3), (50, 0), (300, 7), (4000, 40), (2000, 700)):
        offsets, data, vvalid = random_binary(rng, nvals, odt, mean_len, 0.15 if nvals % 2 == 0 else 0.0)
        for n, idt in ((1, np.int8), (63, np.uint8), (1025, np.int16), (70001, np.int32), (5000, np.uint64)):
            voff = int(rng.integers(0, max(1, nvals // 3)))
            avail = nvals - voff
            hi = min(avail, np.iinfo(idt).max + 1)
            idx = rng.integers(0, hi, n).astype(idt)
            ivalid = OL.pack_bits(list(rng.random(n) >= 0.1)) if n % 2 else None
            want_valid = vvalid is not None or ivalid is not None
            e = orc_be.take_binary(offsets, data, vvalid, voff, avail, idx, ivalid, 0, want_valid)
            g = hip.take_binary(offsets, data, vvalid, voff, avail, idx, ivalid, 0, want_valid)
            assert e[0] == g[0] == STATUS_OK
            assert g[1].tobytes() == e[1].tobytes(), ("offsets", nvals, n, idt)
            assert g[2].tobytes() == e[2].tobytes(), ("data", nvals, n, idt)
            if want_valid:
                assert g[3].tobytes() == e[3].tobytes() and g[4] == e[4]
    # first offending index wins, null index slots are not checked
    idx = np.array([0, 7, 1000, -3, 2000], np.int32)
    ivalid = OL.pack_bits([True, True, False, True, True])
    offsets, data, vvalid = random_binary(rng, 10, odt, 5, 0.0)
    assert hip.take_binary(offsets, data, None, 0, 10, idx, ivalid, 0, True)[0::5] == (STATUS_EINDEX, -3)


@pytest.mark.parametrize("odt", [np.int32, np.int64], ids=["binary", "large_binary"])
def test_filter_binary_bit_exact(hip, orc_be, odt):
    rng = np.random.default_rng(9100 + np.dtype(odt).itemsize)
    for n, mean_len in ((1, 4), (65, 0), (3000, 12), (70001, 9), (20000, 300)):
        offsets, data, vvalid = random_binary(rng, n + 7, odt, mean_len, 0.2 if n % 2 else 0.0)
        voff = 7
        foff = int(rng.integers(0, 30))
        for sel, null_sel, p_fnull in ((0.5, DROP, 0.0), (0.1, EMIT, 0.2), (0.95, DROP, 0.2), (0.0, DROP, 0.0), (1.0, EMIT, 0.0)):
            fd = OL.pack_bits([False] * foff + list(rng.random(n) < sel))
            fv = OL.pack_bits([True] * foff + list(rng.random(n) >= p_fnull)) if p_fnull else None
            want_valid = vvalid is not None or fv is not None
            e = orc_be.filter_binary(offsets, data, vvalid, voff, fd, fv, foff, n, null_sel, want_valid)
            g = hip.filter_binary(offsets, data, vvalid, voff, fd, fv, foff, n, null_sel, want_valid)
            assert g[0].tobytes() == e[0].tobytes() and g[1].tobytes() == e[1].tobytes(), (n, sel, null_sel)
            if want_valid:
                assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3]


# ---- full-size properties (BASELINE.json configs; no oracle pass needed) -------------------
def test_full_size_properties(ctx):
    """C2/C3 sizes (2^27 rows = 1 GiB columns) checked through size-independent
    properties: Σ(a+b) = Σa + Σb (wrapping), filter(all ones) = identity, filter ∘ count,
    take(identity) = identity, take(reverse)∘take(reverse) = identity, sum of a
    permutation is invariant."""
    import arrow_go_amd as ah
    N = ah._native
    n = 1 << 27
    a = ctx.alloc(n * 8); b = ctx.alloc(n * 8); out = ctx.alloc(n * 8)
    # fill on device: a = iota via filter_to_indices trick is overkill; upload in chunks
    chunk = 1 << 24
    rng = np.random.default_rng(99)
    sa = sb = 0
    for i in range(0, n, chunk):
        ca = rng.integers(-2**40, 2**40, chunk, dtype=np.int64)
        cb = rng.integers(-2**40, 2**40, chunk, dtype=np.int64)
        a.upload(ca, i * 8); b.upload(cb, i * 8)
        sa += int(ca.sum()); sb += int(cb.sum())
    assert ctx.sum_int64(a, n) == sa and ctx.sum_int64(b, n) == sb
    ctx.arithmetic(N.INT64, N.OP_ADD, N.SHAPE_AA, a, b, out, n)
    assert ctx.sum_int64(out, n) == sa + sb
    # filter with an all-ones mask is the identity; with the compare mask, count matches
    mask = ctx.alloc(n // 8 + 64)
    mask.memset(0xFF)
    assert ctx.filter_count(mask, None, 0, n, 0) == n
    ctx.filter_primitive(8, a, None, 0, mask, None, 0, n, 0, n, out, None)
    assert ctx.sum_int64(out, n) == sa
    thr = np.array([0], np.int64)
    ctx.comparison(N.CMP_GT, N.SHAPE_AS, N.INT64, a, thr, mask, n, 0)
    n_out = ctx.filter_count(mask, None, 0, n, 0)
    assert n_out == ctx.count_set_bits(mask, 0, n)
    ctx.filter_primitive(8, a, None, 0, mask, None, 0, n, 0, n_out, out, None)
    fs, fc = ctx.cmp_filter_sum_i64(N.CMP_GT, a, None, 0, n, 0)
    assert fc == n_out and ctx.sum_int64(out, n_out) == fs
    # every survivor satisfies the predicate: comparing the output again selects everything
    ctx.comparison(N.CMP_GT, N.SHAPE_AS, N.INT64, out, thr, mask, n_out, 0)
    assert ctx.count_set_bits(mask, 0, n_out) == n_out
    # take with reversed int32 indices twice = identity (sum + spot check)
    idx = ctx.alloc(n * 4)
    for i in range(0, n, chunk):
        idx.upload(np.arange(n - 1 - i, n - 1 - i - chunk, -1, dtype=np.int32), i * 4)
    ctx.take_primitive(8, a, None, 0, n, 4, True, idx, None, 0, n, True, out, None)
    assert ctx.sum_int64(out, n) == sa
    ctx.take_primitive(8, out, None, 0, n, 4, True, idx, None, 0, n, True, b, None)
    assert b.download(np.int64, 1000, 12345 * 8).tobytes() == a.download(np.int64, 1000, 12345 * 8).tobytes()
    # cumulative_sum: last element = Sum; first differences give the input back
    ctx.cumulative_sum(N.INT64, a, None, 0, n, None, False, False, out, None)
    assert out.download(np.int64, 1, (n - 1) * 8)[0] == np.int64(sa)
    ctx.arithmetic(N.INT64, N.OP_SUB, N.SHAPE_AA, out.at(8), out, b, n - 1)   # b[i] = out[i+1] - out[i]
    ctx.comparison(N.CMP_EQ, N.SHAPE_AA, N.INT64, b, a.at(8), mask, n - 1, 0)
    assert ctx.count_set_bits(mask, 0, n - 1) == n - 1
    for buf in (a, b, out, mask, idx):
        buf.free()


def test_beyond_2_31_rows(ctx):
    """The reference's leaves take a 32-bit length (`int len`, _lib/base_arithmetic.cc:238) and are undefined
    past 2^31 − 1 elements; this ABI is int64 throughout.  One-byte columns of 2^31 + 1027 rows through
    add / compare / popcount / filter / cast / cumulative_sum / min_max / is_in, checked by properties."""
    import arrow_go_amd as ah
    N = ah._native
    n = (1 << 31) + 1027
    a = ctx.alloc(n); b = ctx.alloc(n); out = ctx.alloc(2 * n + 64)
    a.memset(3); b.memset(4)
    tail = np.arange(1027, dtype=np.int8) % 100                 # the rows past 2^31 are distinguishable
    a.upload(tail, 1 << 31)
    ctx.arithmetic(N.INT8, N.OP_ADD, N.SHAPE_AA, a, b, out, n)
    assert out.download(np.int8, 1027, 1 << 31).tolist() == (tail + 4).tolist()
    assert out.download(np.int8, 4, (1 << 31) - 4).tolist() == [7, 7, 7, 7]
    mask = ctx.alloc(n // 8 + 64)
    ctx.comparison(N.CMP_GT, N.SHAPE_AS, N.INT8, a, np.array([50], np.int8), mask, n, 0)
    expect = int((tail > 50).sum())
    assert ctx.count_set_bits(mask, 0, n) == expect
    assert ctx.filter_count(mask, None, 0, n, 0) == expect
    ctx.filter_primitive(1, a, None, 0, mask, None, 0, n, 0, expect, out, None)
    assert out.download(np.int8, expect).tolist() == tail[tail > 50].tolist()
    ctx.cast_numeric(N.INT8, N.INT16, a, None, 0, n, False, False, out)
    assert out.download(np.int16, 1027, 2 * (1 << 31)).tolist() == tail.tolist()
    assert ctx.min_max(N.INT8, a, n, np.int8) == (0, 99)
    # running sum in int64 terms: 3·2^31 + Σ tail, observed modulo 256 in the int8 output
    ctx.cumulative_sum(N.INT8, a, None, 0, n, None, False, False, out, None)
    want_last = (3 * (1 << 31) + int(tail.astype(np.int64).sum())) % 256
    assert int(out.download(np.uint8, 1, n - 1)[0]) == want_last
    od = ctx.alloc(n // 8 + 64); ov = ctx.alloc(n // 8 + 64)
    vs = ctx.to_device(np.array([99, 98], np.int8))
    ctx.is_in(1, a, None, 0, n, vs, None, 0, 2, 0, od, ov, 0)
    assert ctx.count_set_bits(od, 0, n) == int(np.isin(tail, [99, 98]).sum()) and ctx.count_set_bits(ov, 0, n) == n
    for buf in (a, b, out, mask, od, ov):
        buf.free()


# ---- unique / dictionary_encode over binary keys -------------------------------------------------
def binary_from_pool(rng, n, odt, pool):
    """rows drawn from a pool of byte strings; Arrow offsets + data"""
    pick = rng.integers(0, len(pool), n)
    lens = np.array([len(pool[j]) for j in pick], np.int64)
    offsets = np.zeros(n + 1, odt)
    offsets[1:] = np.cumsum(lens)
    data = np.frombuffer(b"".join(pool[j] for j in pick), np.uint8) if offsets[-1] else np.zeros(0, np.uint8)
    return offsets, data


@pytest.mark.parametrize("odt", [np.int32, np.int64], ids=["binary", "large_binary"])
def test_hash_binary_encode_first_seen_order(hip, orc_be, odt):
    """ids, index validity, the first row of every dictionary entry and the null id: all identical to the
    sequential memo table — short keys, keys longer than 16 bytes, empty strings, shared prefixes and
    equal lengths (so the byte comparison decides), nulls encoded or masked, sliced input"""
    rng = np.random.default_rng(9100 + np.dtype(odt).itemsize)
    for card, maxlen in ((1, 4), (6, 0), (40, 3), (500, 12), (3000, 40), (20000, 9)):
        pool = [bytes(rng.integers(97, 100, int(rng.integers(0, maxlen + 1)), dtype=np.uint8)) for _ in range(card)]
        pool += [p + b"x" for p in pool[: card // 4]] + [b"", b"a" * 17, b"a" * 16 + b"b", b"a" * 24, b"a" * 23 + b"c"]
        for n in (1, 65, 3001, 150001):
            offsets, data = binary_from_pool(rng, n + 9, odt, pool)
            valid = rand_bits(rng, n + 16, 0.9)
            for off, v in ((0, None), (0, valid), (9, valid)):
                for enc in (True, False):
                    g = hip.hash_binary_encode(offsets, data, v, off, n, enc)
                    e = orc_be.hash_binary_encode(offsets, data, v, off, n, enc)
                    assert g[0].tobytes() == e[0].tobytes(), (card, n, off, enc)
                    assert g[1].tobytes() == e[1].tobytes()
                    assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3]


@pytest.mark.parametrize("w", [3, 16, 32, 7])
def test_hash_fixed_width_keys(hip, orc_be, w):
    """unique / dictionary_encode of FixedSizeBinary (w = 3, 7), Decimal128 (16) and Decimal256 (32) keys — the reference hashes
    them through the same BinaryMemoTable as strings (kernels/vector_hash.go:608-609, 698).  First the reference's own vectors
    (vector_hash_test.go:342-389: ["aaa", null, "bbb", "aaa"] → ["aaa", null, "bbb"]; decimals [12, null, 11, 12] → [12, null, 11]),
    then random columns against the oracle's memo table: ids, index validity, first rows, null id and the dictionary bytes."""
    if w == 3:
        data = np.frombuffer(b"aaa" + b"zzz" + b"bbb" + b"aaa", np.uint8)
        valid = np.array([0b1101], np.uint8)
        for be in (hip, orc_be):
            ids, idv, first, nid, dic = be.hash_fixed_encode(data, 3, valid, 0, 4, True)
            assert ids.tolist() == [0, 1, 2, 0] and nid == 1 and first.tolist() == [0, 1, 2] and bytes(dic) == b"aaa\0\0\0bbb"
    if w in (16, 32):
        num = lambda v: np.frombuffer(int(v).to_bytes(w, "little", signed=True), np.uint8)
        data = np.concatenate([num(12), num(12), num(11), num(12)])       # slot 1 is null: its bytes must not matter
        valid = np.array([0b1101], np.uint8)
        for be in (hip, orc_be):
            ids, idv, first, nid, dic = be.hash_fixed_encode(data, w, valid, 0, 4, True)
            assert ids.tolist() == [0, 1, 2, 0] and nid == 1
            assert bytes(dic) == bytes(num(12)) + bytes(w) + bytes(num(11))
    rng = np.random.default_rng(9300 + w)
    for card, n in ((1, 1), (5, 70), (300, 3001), (20000, 150001)):
        pool = rng.integers(0, 4, (card, w), dtype=np.uint8)       # few symbols: many shared prefixes, the byte comparison decides
        data = pool[rng.integers(0, card, n + 9)].reshape(-1)
        valid = rand_bits(rng, n + 16, 0.9)
        for off, v in ((0, None), (0, valid), (9, valid)):
            for enc in (True, False):
                g, e = hip.hash_fixed_encode(data, w, v, off, n, enc), orc_be.hash_fixed_encode(data, w, v, off, n, enc)
                assert g[0].tobytes() == e[0].tobytes(), (w, card, n, off, enc)
                assert g[1].tobytes() == e[1].tobytes() and g[2].tobytes() == e[2].tobytes() and g[3] == e[3]
                assert g[4].tobytes() == e[4].tobytes()


def test_hash_binary_encode_large(hip, orc_be):
    # beyond the 2^21-row prefix: direct ids for keys the prefix knew, late keys, table growth
    rng = np.random.default_rng(9200)
    n = (1 << 22) + 321
    pool = [b"k%07d" % i for i in range(5000)]
    offsets, data = binary_from_pool(rng, n, np.int32, pool)
    valid = rand_bits(rng, n + 8, 0.95)
    for enc in (True, False):
        g, e = hip.hash_binary_encode(offsets, data, valid, 0, n, enc), orc_be.hash_binary_encode(offsets, data, valid, 0, n, enc)
        assert g[0].tobytes() == e[0].tobytes() and g[1].tobytes() == e[1].tobytes()
        assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3]
    # mostly distinct 8-byte values: the table is re-planned
    n = (1 << 22) + 5
    data = rng.integers(0, 256, n * 8, dtype=np.uint8)
    offsets = (np.arange(n + 1, dtype=np.int64) * 8)
    g, e = hip.hash_binary_encode(offsets, data, None, 0, n, True), orc_be.hash_binary_encode(offsets, data, None, 0, n, True)
    assert g[0].tobytes() == e[0].tobytes() and g[2].tobytes() == e[2].tobytes()


# ---- divide / shifts / bit-wise / abs / negate / sqrt ------------------------------------------------
_XOPS = dict(DIV=3, SQRT=6, DIV_CHECKED=24, ABS_CHECKED=25, NEGATE_CHECKED=26, SQRT_CHECKED=27, SHL=64, SHL_CHECKED=65, SHR=66,
             SHR_CHECKED=67, AND=68, OR=69, XOR=70, NOT=71)


def _ext_same(g, e, what):
    assert g[0] == e[0], (what, g[2], e[2])
    if e[0] == 0:
        assert g[1].tobytes() == e[1].tobytes(), what      # every byte, null slots included
    else:
        assert g[2].endswith(e[2]) or e[2] in g[2], (what, g[2], e[2])


@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64], ids=str)
def test_arithmetic_ext_integers_bit_exact(hip, orc_be, dtype):
    rng = np.random.default_rng(1200 + np.dtype(dtype).itemsize * 2 + (np.iinfo(dtype).min < 0))
    info = np.iinfo(dtype)
    for n in (1, 15, 16, 17, 1000, 70001):
        a = rng.integers(info.min, info.max, n + 9, dtype=dtype, endpoint=True)
        b = rng.integers(info.min, info.max, n + 9, dtype=dtype, endpoint=True)
        b[b == 0] = 1
        small = rng.integers(-2 if info.min < 0 else 0, info.bits + 2, n + 9).astype(dtype)   # shift counts around the legal range
        lv, rv = rand_bits(rng, n + 16, 0.85), rand_bits(rng, n + 16, 0.85)
        for sl in (0, 3):   # element-aligned but not 16-byte aligned slices
            A, B, S = a[sl:sl + n], b[sl:sl + n], small[sl:sl + n]
            for op in ("DIV", "DIV_CHECKED"):
                for shape, l, r in ((0, A, B), (1, A, B[:1]), (2, A[:1], B)):
                    _ext_same(hip.arithmetic_ext(_XOPS[op], shape, l, lv, sl, r, rv, 5), orc_be.arithmetic_ext(_XOPS[op], shape, l, lv, sl, r, rv, 5), (op, n, shape))
            # a zero divisor: an error when its slot is valid, ignored under a null
            Bz = B.copy(); Bz[n // 2] = 0
            for v in (None, rv):
                _ext_same(hip.arithmetic_ext(_XOPS["DIV"], 0, A, None, 0, Bz, v, 5), orc_be.arithmetic_ext(_XOPS["DIV"], 0, A, None, 0, Bz, v, 5), ("div0", n))
            legal = (S.astype(np.int64) % (info.bits - 1)).astype(dtype)
            for op in ("SHL", "SHR", "SHL_CHECKED", "SHR_CHECKED"):
                counts = legal if op.endswith("CHECKED") else S
                for shape, l, r in ((0, A, counts), (1, A, counts[:1]), (2, A[:1], counts)):
                    _ext_same(hip.arithmetic_ext(_XOPS[op], shape, l, lv, sl, r, rv, 5), orc_be.arithmetic_ext(_XOPS[op], shape, l, lv, sl, r, rv, 5), (op, n, shape))
                _ext_same(hip.arithmetic_ext(_XOPS[op], 0, A, None, 0, S, rv, 5), orc_be.arithmetic_ext(_XOPS[op], 0, A, None, 0, S, rv, 5), (op, "illegal counts", n))
            for op in ("AND", "OR", "XOR"):
                for shape, l, r in ((0, A, B), (1, A, B[:1]), (2, A[:1], B)):
                    _ext_same(hip.arithmetic_ext(_XOPS[op], shape, l, lv, sl, r, rv, 5), orc_be.arithmetic_ext(_XOPS[op], shape, l, lv, sl, r, rv, 5), (op, n, shape))
            _ext_same(hip.arithmetic_ext(_XOPS["NOT"], 1, A, lv, sl, None, None, 0), orc_be.arithmetic_ext(_XOPS["NOT"], 1, A, lv, sl, None, None, 0), ("not", n))
            ops = ("ABS_CHECKED", "NEGATE_CHECKED") if info.min < 0 else ("ABS_CHECKED",)
            for op in ops:
                An = A.copy(); An[An == info.min] = 0
                _ext_same(hip.arithmetic_ext(_XOPS[op], 1, An, lv, sl, None, None, 0), orc_be.arithmetic_ext(_XOPS[op], 1, An, lv, sl, None, None, 0), (op, n))
                if info.min < 0:
                    Am = An.copy(); Am[n - 1] = info.min
                    _ext_same(hip.arithmetic_ext(_XOPS[op], 1, Am, lv, sl, None, None, 0), orc_be.arithmetic_ext(_XOPS[op], 1, Am, lv, sl, None, None, 0), (op, "min", n))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=str)
def test_arithmetic_ext_floats_bit_exact(hip, orc_be, dtype):
    """one correctly rounded IEEE operation per element: bit-exact, NaN / Inf / signed zeros / denormals included"""
    rng = np.random.default_rng(1300 + np.dtype(dtype).itemsize)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, np.finfo(dtype).tiny, np.finfo(dtype).tiny / 8, np.finfo(dtype).max], dtype)
    for n in (1, 7, 1000, 70001):
        a = (rng.standard_normal(n + 5) * 10.0 ** rng.integers(-30, 30, n + 5)).astype(dtype)
        b = (rng.standard_normal(n + 5) * 10.0 ** rng.integers(-30, 30, n + 5)).astype(dtype)
        k = min(len(special), n)
        a[:k] = special[:k]; b[:k] = special[::-1][:k]
        lv, rv = rand_bits(rng, n + 16, 0.85), rand_bits(rng, n + 16, 0.85)
        with np.errstate(all="ignore"):
            for sl in (0, 1):
                A, B = a[sl:sl + n], b[sl:sl + n]
                for shape, l, r in ((0, A, B), (1, A, B[:1]), (2, A[:1], B)):
                    _ext_same(hip.arithmetic_ext(_XOPS["DIV"], shape, l, lv, sl, r, rv, 5), orc_be.arithmetic_ext(_XOPS["DIV"], shape, l, lv, sl, r, rv, 5), ("div", n, shape))
                Bn = B.copy(); Bn[Bn == 0] = 2
                _ext_same(hip.arithmetic_ext(_XOPS["DIV_CHECKED"], 0, A, lv, sl, Bn, rv, 5), orc_be.arithmetic_ext(_XOPS["DIV_CHECKED"], 0, A, lv, sl, Bn, rv, 5), ("divc", n))
                _ext_same(hip.arithmetic_ext(_XOPS["DIV_CHECKED"], 0, A, None, 0, B, None, 0), orc_be.arithmetic_ext(_XOPS["DIV_CHECKED"], 0, A, None, 0, B, None, 0), ("divc zero", n))
                for op in ("ABS_CHECKED", "NEGATE_CHECKED", "SQRT"):
                    _ext_same(hip.arithmetic_ext(_XOPS[op], 1, A, lv, sl, None, None, 0), orc_be.arithmetic_ext(_XOPS[op], 1, A, lv, sl, None, None, 0), (op, n))
                P = np.abs(A)
                _ext_same(hip.arithmetic_ext(_XOPS["SQRT_CHECKED"], 1, P, lv, sl, None, None, 0), orc_be.arithmetic_ext(_XOPS["SQRT_CHECKED"], 1, P, lv, sl, None, None, 0), ("sqrtc", n))
                _ext_same(hip.arithmetic_ext(_XOPS["SQRT_CHECKED"], 1, A, None, 0, None, None, 0), orc_be.arithmetic_ext(_XOPS["SQRT_CHECKED"], 1, A, None, 0, None, None, 0), ("sqrtc neg", n))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=str)
def test_round_bit_exact(hip, orc_be, dtype):
    rng = np.random.default_rng(1400 + np.dtype(dtype).itemsize)
    n = 50021
    x = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, n)).astype(dtype)
    x[:8] = [0.5, 1.5, 2.5, -0.5, -1.5, np.inf, -np.inf, np.nan]
    x[8:16] = np.array([0.125, 0.375, 2.675, -2.675, 1e15, -1e15, 0.0, -0.0], dtype)
    valid = rand_bits(rng, n + 8, 0.9)
    for mode in range(10):
        for nd in (-3, -1, 0, 1, 2, 5):
            for v, off in ((None, 0), (valid, 3)):
                g, e = hip.round(x, v, off, nd, mode), orc_be.round(x, v, off, nd, mode)
                assert g[0] == e[0] == 0 and g[1].tobytes() == e[1].tobytes(), (mode, nd)
        for mult in (0.05, 0.1, 0.25, 2, 7, 1000):
            g, e = hip.round(x, valid, 3, 0, mode, multiple=mult), orc_be.round(x, valid, 3, 0, mode, multiple=mult)
            assert g[0] == e[0] == 0 and g[1].tobytes() == e[1].tobytes(), (mode, mult)


# ---- ShiftTime (temporal unit casts) -------------------------------------------------------------------------------
@pytest.mark.parametrize("in_t,out_t", [(np.int32, np.int32), (np.int32, np.int64), (np.int64, np.int32), (np.int64, np.int64)],
                         ids=["32to32", "32to64", "64to32", "64to64"])
def test_shift_time_bit_exact(hip, orc_be, in_t, out_t):
    """multiply / divide, checked and not, all four width pairs: same integers in every slot (null slots included), the same
    first offending value when a check fires, offenders under null slots ignored; sizes cross the 4-row lane tile, buffers
    are misaligned to force the scalar path."""
    rng = np.random.default_rng(8100 + np.dtype(in_t).itemsize * 10 + np.dtype(out_t).itemsize)
    info = np.iinfo(in_t)
    for k, n in enumerate([1, 3, 4, 5, 1023, 1024, 1025, 65537, 1 << 20]):
        for factor in [1, 1000, 86400000]:
            wide = rng.integers(info.min, info.max, n, dtype=in_t, endpoint=True)
            small = (rng.integers(-1000, 1000, n) * min(factor, 1000)).astype(in_t)   # passes both checks
            valid = OL.pack_bits(rng.random(n + 5) < 0.8)
            for op in (0, 1):
                # unchecked: every slot computed, wrapping / truncating
                st_e, e, _ = orc_be.shift_time(wide, out_t, op, factor, False, valid, 5)
                st_g, g, _ = hip.shift_time(wide, out_t, op, factor, False, valid, 5, misalign=k % 3)
                assert st_e == st_g == STATUS_OK and np.array_equal(e, g), (n, factor, op)
                # checked on values that may or may not pass: same verdict, same first offender
                for vals in (small, wide):
                    st_e, e, bad_e = orc_be.shift_time(vals, out_t, op, factor, True, valid, 5)
                    st_g, g, bad_g = hip.shift_time(vals, out_t, op, factor, True, valid, 5, misalign=(k + 1) % 3)
                    assert st_e == st_g, (n, factor, op)
                    if st_e == STATUS_OK:
                        assert np.array_equal(e, g), (n, factor, op)
                    else:
                        assert bad_e == bad_g, (n, factor, op)
                # all valid
                st_e, e, bad_e = orc_be.shift_time(small, out_t, op, factor, True)
                st_g, g, bad_g = hip.shift_time(small, out_t, op, factor, True)
                assert st_e == st_g and bad_e == bad_g and (st_e != STATUS_OK or np.array_equal(e, g)), (n, factor, op)


def test_shift_time_full_size_round_trip(hip):
    """at a bench-sized column: s → ns → s is the identity, and the ns values are the seconds times 10^9 (linearity checked by sum)"""
    rng = np.random.default_rng(8200)
    n = 1 << 24
    secs = rng.integers(-2**31, 2**31, n).astype(np.int64)
    st, ns, _ = hip.shift_time(secs, np.int64, 0, 1000000000, True)
    assert st == STATUS_OK and (int(ns.sum()) - int(secs.sum()) * 1000000000) % 2**64 == 0   # numpy's int64 sum wraps
    st, back, _ = hip.shift_time(ns, np.int64, 1, 1000000000, True)
    assert st == STATUS_OK and np.array_equal(back, secs)


# ---- power -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64], ids=str)
def test_power_integers_bit_exact(hip, orc_be, dtype):
    """power_unchecked wraps like the uint64 square-and-multiply of the reference in every slot; power reports exactly the
    overflows mulWithOverflow would and skips null slots; negative exponents are refused by both (by the unchecked form even
    under a null)."""
    info = np.iinfo(dtype)
    rng = np.random.default_rng(9100 + info.bits + (info.min < 0))
    for n in (1, 15, 16, 17, 1000, 70001):
        base = rng.integers(info.min, info.max, n + 4, dtype=dtype, endpoint=True)
        base[rng.random(n + 4) < 0.5] = rng.integers(max(info.min, -3), 4)          # small bases: results that fit
        exp = rng.integers(0, min(info.max, 70), n + 4).astype(dtype)
        lv, rv = rand_bits(rng, n + 16, 0.85), rand_bits(rng, n + 16, 0.85)
        for sl in (0, 3):
            A, E = base[sl:sl + n], exp[sl:sl + n]
            for shape, l, r in ((0, A, E), (1, A, E[:1]), (2, A[:1], E)):
                _ext_same(hip.arithmetic_ext(7, shape, l, lv, sl, r, rv, 5), orc_be.arithmetic_ext(7, shape, l, lv, sl, r, rv, 5), ("pow", n, shape))
            # checked: exponents small enough that nothing overflows, then the general case (usually "overflow")
            tiny = (E.astype(np.int64) % 3).astype(dtype)
            fits = np.clip(A.astype(np.float64), -11, 11).astype(dtype) if info.bits >= 16 else np.clip(A.astype(np.float64), -5, 5).astype(dtype)
            _ext_same(hip.arithmetic_ext(28, 0, fits, lv, sl, tiny, rv, 5), orc_be.arithmetic_ext(28, 0, fits, lv, sl, tiny, rv, 5), ("powc fits", n))
            _ext_same(hip.arithmetic_ext(28, 0, A, lv, sl, E, rv, 5), orc_be.arithmetic_ext(28, 0, A, lv, sl, E, rv, 5), ("powc", n))
            _ext_same(hip.arithmetic_ext(28, 1, fits, lv, sl, tiny[:1], None, 0), orc_be.arithmetic_ext(28, 1, fits, lv, sl, tiny[:1], None, 0), ("powc AS", n))
            if info.min < 0:
                En = E.copy(); En[n // 2] = -1
                for op in (7, 28):
                    for v in (None, rv):
                        _ext_same(hip.arithmetic_ext(op, 0, fits, None, 0, En, v, 5), orc_be.arithmetic_ext(op, 0, fits, None, 0, En, v, 5), ("neg exp", op, n))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=str)
def test_power_floats_close(hip, orc_be, dtype):
    """math.Pow is not correctly rounded and neither is the device's pow; the reference's own test is ApproxEqual.
    Tolerance: 4 ulp of the type against the host libm, special values (NaN, ±Inf, ±0, 1) exactly."""
    rng = np.random.default_rng(9200 + np.dtype(dtype).itemsize)
    n = 50001
    a = np.abs(rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(dtype)
    b = (rng.standard_normal(n) * 4).astype(dtype)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 2.0, 0.5, -2.0], dtype)
    a[:10] = special; b[:10] = special[::-1]
    a[10:20] = special; b[10:20] = np.array([0, 1, 2, -1, 0.5, np.inf, -np.inf, np.nan, 3, 3], dtype)
    with np.errstate(all="ignore"):
        for op in (7, 28):
            g, e = hip.arithmetic_ext(op, 0, a, None, 0, b, None, 0), orc_be.arithmetic_ext(op, 0, a, None, 0, b, None, 0)
            assert g[0] == e[0] == 0
            G, E = g[1].astype(np.float64), e[1].astype(np.float64)
            assert np.array_equal(np.isnan(G), np.isnan(E))
            fin = np.isfinite(E)
            assert np.array_equal(G[~fin & ~np.isnan(E)], E[~fin & ~np.isnan(E)])
            assert np.all(np.abs(G[fin] - E[fin]) <= 4 * np.finfo(dtype).eps * np.abs(E[fin]) + np.finfo(dtype).tiny), np.max(np.abs(G[fin] - E[fin]) / np.maximum(np.abs(E[fin]), 1e-300))


def test_graph_capture_replays_a_chain():
    """ah_graph_begin / _end / _launch: an Add → Compare → bitmap AND → fused compare-filter-sum → Sum chain over a small column is
    recorded once and replayed with new contents under the same pointers; every replay equals numpy on the contents of that
    moment, and a call that has to wait for the device invalidates the capture instead of running half a sequence."""
    import arrow_go_amd as ah
    N = ah._native
    ctx = ah.Context(0)      # its own context: the last part needs work areas that have not grown yet
    rng = np.random.default_rng(77)
    n = (1 << 16) + 77
    thr = np.array([5], np.int64)
    da, db = ctx.alloc(n * 8), ctx.alloc(n * 8)
    dc = ctx.alloc(n * 8)
    dmask, dother, dand = ctx.alloc(n // 8 + 64), ctx.alloc(n // 8 + 64), ctx.alloc(n // 8 + 64)
    dfused, dsum = ctx.alloc(16), ctx.alloc(8)
    other = rng.integers(0, 256, n // 8 + 64, dtype=np.uint8)
    dother.upload(other)

    def chain():
        ctx.arithmetic(N.INT64, N.OP_ADD, N.SHAPE_AA, da, db, dc, n)
        ctx.comparison(N.CMP_GT, N.SHAPE_AS, N.INT64, dc, thr, dmask, n, 0)
        ctx.bitmap_op(N.BIT_AND, dmask, 0, dother, 0, dand, 0, n)
        ctx.cmp_filter_sum_i64_dev(N.CMP_GT, dc, dother, 0, n, int(thr[0]), dfused)
        ctx.sum_int64_dev(dc, n, dsum)

    def check_against(a, b):
        c = a + b
        obits = np.unpackbits(other, bitorder="little")[:n].astype(bool)
        assert dc.download(np.int64, n).tobytes() == c.tobytes()
        got = np.unpackbits(dand.download(np.uint8, (n + 7) // 8), bitorder="little")[:n].astype(bool)
        assert np.array_equal(got, (c > thr[0]) & obits)
        fs = dfused.download(np.int64, 2)
        sel = (c > thr[0]) & obits
        assert int(fs[0]) == int(c[sel].sum()) and int(fs[1]) == int(sel.sum())
        assert int(dsum.download(np.int64, 1)[0]) == int(c.sum())

    a = rng.integers(-1000, 1000, n, dtype=np.int64); b = rng.integers(-1000, 1000, n, dtype=np.int64)
    da.upload(a); db.upload(b)
    chain()                                  # eager warm-up: the scratch arenas get their size
    check_against(a, b)
    ctx.graph_begin()
    chain()
    g = ctx.graph_end()
    for seed in (1, 2, 3):
        r2 = np.random.default_rng(seed)
        a = r2.integers(-1000, 1000, n, dtype=np.int64); b = r2.integers(-1000, 1000, n, dtype=np.int64)
        da.upload(a); db.upload(b)
        dc.memset(0); dand.memset(0); dfused.memset(0); dsum.memset(0)
        g.launch()
        check_against(a, b)
    # a larger call grows the context's scratch area: the graph's launches would point into the freed block — refused
    big = rng.integers(0, 1 << 20, 1 << 22, dtype=np.int64)
    dk, di, dd = ctx.to_device(big), ctx.alloc(big.size * 4), ctx.alloc((big.size + 1) * 8)
    ctx.hash_u64_encode(dk, None, 0, big.size, False, di, None, dd)
    with pytest.raises(ah.ArrowHipError, match="record the sequence again"):
        g.launch()
    g.close()
    for d in (dk, di, dd):
        d.free()
    # a call with a host result cannot be recorded: the capture is dropped, the context stays usable
    ctx.graph_begin()
    with pytest.raises(ah.ArrowHipError):
        ctx.sum_int64(dc, n)
        ctx.graph_end()
    try:
        ctx.graph_end()
    except ah.ArrowHipError:
        pass
    assert ctx.sum_int64(dc, n) == int((a + b).sum())
    for d in (da, db, dc, dmask, dother, dand, dfused, dsum):
        d.free()
    ctx.close()


# ---- the streaming-reduction layer (ah_reduce.h): Sum, fused filter-sum, min_max, popcount, the sort's key statistics -------------
REDUCE_SETTINGS = [(bpc, nt) for bpc in (1, 2, 8) for nt in (0, 1)]
# rows of 8-byte types: one walk iteration of 256 × 4 vectors of two rows, ± 1 (a head row when misaligned); 2^20 makes the
# grid-stride loop wrap at one workgroup per CU
REDUCE_SIZES = [1, 2, 3, 2047, 2048, 2049, 2050, 4097, 1 << 20]


def _with_reduce_settings(ctx, run):
    """run() under every (blocks_per_cu, nt) setting → the list of its results; the context's own settings come back afterwards"""
    import os
    try:
        out = []
        for bpc, nt in REDUCE_SETTINGS:
            ctx.set_option("blocks_per_cu", bpc)
            ctx.set_option("nt", nt)
            out.append(run())
        return out
    finally:
        ctx.set_option("blocks_per_cu", int(os.environ.get("ARROWHIP_BLOCKS_PER_CU", 0)))
        ctx.set_option("nt", int(os.environ.get("ARROWHIP_NT", 1)))


def test_reductions_are_independent_of_grid_and_hint(ctx, orc_be):
    """Sum, the fused filter-sum, min_max and the popcount return the oracle's answer whatever the grid (1, 2, 8 workgroups per CU)
    and with or without the nontemporal hint: the walk, the workgroup reduction and the finish they share leave no row out and
    count none twice at any of the sizes around one walk iteration."""
    import arrow_go_amd as ah
    N = ah._native
    rng = np.random.default_rng(9100)

    def check(what, run, want):
        got = _with_reduce_settings(ctx, run)
        assert all(g == want for g in got), (what, got, want)

    for n in REDUCE_SIZES:
        raw = rng.integers(0, 2**64 - 1, n, dtype=np.uint64, endpoint=True)
        ints = rng.integers(-2**40, 2**40, n).astype(np.float64)          # integer-valued doubles: exact in any order
        x = rng.integers(-10**9, 10**9, n, dtype=np.int64)
        valid = rand_bits(rng, n + 5, 0.9)
        dvalid = ctx.to_device(valid)
        want_sum_f64 = float(ints.astype(np.int64).sum())
        want_fused = orc_be.cmp_filter_sum_i64(GT, x, None, 0, 0), orc_be.cmp_filter_sum_i64(GT, x, valid, 5, 0)
        for misalign in (0, 1):
            lead = 8 * misalign
            draw, dints, dx = ctx.alloc(lead + 8 * n + 64), ctx.alloc(lead + 8 * n + 64), ctx.alloc(lead + 8 * n + 64)
            draw.upload(raw, lead); dints.upload(ints, lead); dx.upload(x, lead)
            what = (n, misalign)
            check(("sum_int64",) + what, lambda: ctx.sum_int64(draw.ptr + lead, n), orc_be.sum(raw.view(np.int64)))
            check(("sum_uint64",) + what, lambda: ctx.sum_uint64(draw.ptr + lead, n), orc_be.sum(raw))
            check(("sum_float64",) + what, lambda: ctx.sum_float64(dints.ptr + lead, n), want_sum_f64)
            check(("fused",) + what, lambda: ctx.cmp_filter_sum_i64(GT, dx.ptr + lead, None, 0, n, 0), want_fused[0])
            check(("fused, validity",) + what, lambda: ctx.cmp_filter_sum_i64(GT, dx.ptr + lead, dvalid, 5, n, 0), want_fused[1])
            for dt in OL.INT_DTYPES:   # the same bytes as rows of every width
                v = raw.view(dt)
                check(("min_max", str(dt)) + what, lambda: ctx.min_max(OL.TYPE_IDS[dt], draw.ptr + lead, v.size, dt), orc_be.min_max(v))
            for d in (draw, dints, dx):
                d.free()
        dvalid.free()
    for n in (15, 16, 17, 16383, 16384, 16385, 16400):   # 1-byte rows: 16 per vector
        for dt in (np.dtype(np.int8), np.dtype(np.uint8)):
            v = rand(rng, dt, n)
            for misalign in (0, 1):
                d = ctx.alloc(misalign + n + 64)
                d.upload(v, misalign)
                check(("min_max", str(dt), n, misalign), lambda: ctx.min_max(OL.TYPE_IDS[dt], d.ptr + misalign, n, dt), orc_be.min_max(v))
                d.free()
    bits = rand_bits(rng, 300007 + 65)
    dbits = ctx.to_device(bits)
    for off in (0, 1, 7, 63, 64, 65):
        for nbits in (1, 63, 64, 65, 65535, 65536, 65537, 300007):
            check(("popcount", off, nbits), lambda: ctx.count_set_bits(dbits, off, nbits), orc_be.count_set_bits(bits, off, nbits))
    dbits.free()


@pytest.mark.parametrize("dtype", OL.INT_DTYPES, ids=str)
def test_min_max_sizes_and_alignment(hip, orc_be, dtype):
    """the extreme values in every place the kernel treats differently: the head rows before the 16-byte-aligned body, the tail rows
    after it, the first and the last vector of the body, and the last row of the ragged walk iteration"""
    dt = np.dtype(dtype)
    info = np.iinfo(dt)
    V = 16 // dt.itemsize
    rng = np.random.default_rng(9200 + OL.TYPE_IDS[dt])
    mid_lo, mid_hi = info.min // 2, info.max // 2
    for nvec in (1, 3, 1023, 1024, 1025, 2 * 1024 + 7):   # vectors of the body: below, at and past one walk iteration of 256 × 4
        for misalign in (0, 1):
            head = (V - misalign) % V if misalign else 0    # rows before the first aligned vector
            tail = V - 1
            n = head + nvec * V + tail
            base = rng.integers(mid_lo, mid_hi, n, dtype=dt, endpoint=True)
            places = {"first body vector": head, "last body vector": head + (nvec - 1) * V, "tail row": n - 1}
            if nvec % 1024:   # the body's last vector sits in the ragged iteration
                places["last row of the ragged iteration"] = head + nvec * V - 1
            if nvec >= 1024:
                places["last row of the last full iteration"] = head + (nvec // 1024) * 1024 * V - 1
            if head:
                places["head row"] = 0
            for where, i in places.items():
                for j in (i, n - 1 - i):   # min at the place and max at its mirror image, then the other way round
                    a = base.copy()
                    a[i], a[j] = info.min, info.max
                    want = orc_be.min_max(a)
                    assert (want[0] == info.min or i == j) and want[1] == info.max
                    assert hip.min_max(a, misalign) == want, (dtype, nvec, misalign, where)
                    a[i], a[j] = info.max, info.min
                    assert hip.min_max(a, misalign) == orc_be.min_max(a), (dtype, nvec, misalign, where)
    assert hip.min_max(np.zeros(0, dt)) == orc_be.min_max(np.zeros(0, dt)) == (info.max, info.min)


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 1])
def test_sort_indices_key_statistics(hip, orc_be, n):
    """From 2^20 rows on a column without validity takes the one-pass key + statistics kernel (AND / OR / min / max of the keys and the
    NaN count per workgroup, folded by the host).  Keys that differ only in bits 40–47: the passes the sort runs are chosen from those
    statistics, and a wrong AND / OR would skip the one byte that matters; the Float64 column's one NaN, in the last row, must send it
    down the partition path."""
    rng = np.random.default_rng(9300 + n)
    byte5 = rng.integers(0, 256, n, dtype=np.int64) << 40
    ints = (np.int64(0x1234) << 48) + byte5 + 0x89ABCDEF01
    flts = ((np.int64(0x4012) << 48) + byte5 + 0x89ABCDEF01).view(np.float64).copy()
    flts[n - 1] = np.nan
    for a in (ints, flts):
        for desc in (False, True):
            e = orc_be.sort_indices(a, None, 0, desc, False)
            g = hip.sort_indices(a, None, 0, desc, False)
            assert g.tobytes() == e.tobytes(), (a.dtype, n, desc)
