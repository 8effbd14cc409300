"""Kernels write only the bytes they own, at any alignment.

tests/backends.py::HipBackend allocates every output as a GuardedBuffer: exactly the bytes include/arrowhip.h gives the output,
between two 4 KiB bands that must come back unchanged.  This file tests the guard itself (against an in-memory stand-in without a
GPU, with one stray byte on a real buffer with one), then sweeps the primitive kernels over the smallest shapes at which a vector
kernel's head and tail can go wrong: every output phase of a 16-byte line, input phases independent of it, lengths around one
vector, one wave of vectors and one block iteration — or around one tile of the compacting / gathering kernels.  Expected values
come from the oracle backend and are compared byte for byte; the bands are checked inside HipBackend after every call.

Not reached at these shapes: the clustered Take (chosen by a neighbour sample of columns ≥ 64 MiB) and the MSD sort (≥ 2^20 rows).
"""
import os
import re

import numpy as np
import pytest

from tests import oracle_lib as OL
from tests.backends import GUARD_BAND, GUARD_FILL, GuardedBuffer, HipBackend, OracleBackend, STATUS_OK
from tests.test_gpu_parity import _XOPS, _ext_same, cast_input, rand, rand_bits, random_binary, same_bits_or_both_nan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow_go_amd", "csrc")

ADD, SUB, MUL = 0, 1, 2
AA, AS, SA = 0, 1, 2
DROP, EMIT = 0, 1

# rows per workgroup step of the compacting / gathering kernels (test_the_tiles_are_the_kernels_tiles reads them from the source)
FILTER_TILE_BYTES = 16384                 # ah_filter.hip: a tile is 16 KiB of values, 16384 / w rows
TAKE_TILE = 256 * 4                       # ah_take.hip: kBlock lanes × AH_TAKE_UNROLL rows
VARLEN_TILE = 256                         # ah_varlen.hip: one row per lane
SORT_TILE = 256 * 8                       # ah_sort_radix.h: kTile = kBlock × kItems
HASH_TILE = 1024 * 8                      # ah_hash.hip: kSmallBlock lanes × kSmallRows rows
BOOL_CAST_BLOCK = 256                     # ah_cast_impl.h: one 16-byte vector per lane, 256 · V rows
SCAN_ONEPASS_ROWS = 1 << 18               # ah_scan.hip: 16-byte aligned 2- / 4- / 8-byte columns from here on take the one-pass kernels


def scan_tile(w):
    """ah_scan.hip, Geom<T, VPT>::TILE: 4 waves × 64 lanes × VPT vectors × V rows, VPT = 8 for 4- / 8-byte rows, else 4"""
    return 4 * 64 * (8 if w >= 4 else 4) * (16 // w)


@pytest.fixture(scope="module")
def hip(ctx):
    return HipBackend(ctx, dirty_outputs=True)


@pytest.fixture(scope="module")
def orc_be():
    return OracleBackend()


# ---- no GPU needed: the guard against an in-memory stand-in ----------------------------------------------------------------------------
class _HostBuf:
    def __init__(self, ctx, ptr, nbytes):
        self.ctx, self.ptr, self.nbytes, self.data = ctx, ptr, nbytes, bytearray(nbytes)

    def upload(self, arr, byte_offset=0):
        b = np.ascontiguousarray(arr).tobytes()
        assert byte_offset + len(b) <= self.nbytes
        self.data[byte_offset:byte_offset + len(b)] = b
        return self

    def download(self, dtype, count, byte_offset=0):
        nb = int(count) * np.dtype(dtype).itemsize
        assert byte_offset + nb <= self.nbytes
        return np.frombuffer(bytes(self.data[byte_offset:byte_offset + nb]), dtype=dtype).copy()

    def memset(self, byte_value, nbytes=None, byte_offset=0):
        nbytes = self.nbytes if nbytes is None else nbytes
        assert byte_offset + nbytes <= self.nbytes
        self.data[byte_offset:byte_offset + nbytes] = bytes([byte_value]) * nbytes

    def free(self):
        self.ctx.freed.append(self.ptr)
        self.ptr = 0


class _HostCtx:
    """alloc / upload / download / memset over bytearrays; pointers are 256-byte aligned like the device allocator's"""
    handle = None

    def __init__(self):
        self.next, self.freed, self.bufs = 0x7000_0000_0000, [], []

    def alloc(self, nbytes):
        b = _HostBuf(self, self.next, nbytes)
        self.next += (nbytes + 255) // 256 * 256 + 256
        self.bufs.append(b)
        return b


def _stray_cases(nbytes, lead):
    """(name, offset of the stray byte inside the whole allocation, side, distance from the payload's edge)"""
    first = GUARD_BAND + lead
    return [("directly in front", first - 1, "front", 1),
            ("directly behind", first + nbytes, "back", 1),
            ("first byte of the front band", 0, "front", first),
            ("last byte of the back band", first + nbytes + GUARD_BAND - 1, "back", GUARD_BAND)]


def _check_guard_reports(ctx, poke):
    """the guard stays quiet for writes inside the payload and names side and distance of one stray byte; poke(raw, offset) changes
    one byte of the allocation"""
    for nbytes, lead in [(37, 0), (37, 5), (0, 0), (4096, 12)]:
        g = GuardedBuffer(ctx, nbytes, lead, "out_values")
        assert g.nbytes == nbytes and g.ptr == g.base + GUARD_BAND + lead
        if nbytes:
            g.memset(0xCD)
            g.upload(np.arange(nbytes, dtype=np.uint8))
            assert g.download(np.uint8, nbytes).tobytes() == np.arange(nbytes, dtype=np.uint8).tobytes()
            g.memset(0x00, 1, nbytes - 1)
            assert g.download(np.uint8, 1, nbytes - 1)[0] == 0
        assert g.changed() is None
        g.check("ah_anything")
        g.free()
        for name, at, side, dist in _stray_cases(nbytes, lead):
            g = GuardedBuffer(ctx, nbytes, lead, "out_values")
            poke(g._raw, at)
            assert g.changed() == (side, dist), (name, nbytes, lead)
            with pytest.raises(AssertionError) as e:
                g.check("ah_some_entry")
            msg = str(e.value)
            assert "ah_some_entry" in msg and "out_values" in msg and f"{side} band" in msg and f"byte {dist} " in msg, (name, msg)
            g.free()


def test_guard_on_the_stand_in():
    _check_guard_reports(_HostCtx(), lambda raw, at: raw.memset(0x00, 1, at))


def test_guard_bands_hold_the_fill_and_the_payload_does_not_need_to():
    ctx = _HostCtx()
    g = GuardedBuffer(ctx, 21, 3)
    raw = bytes(g._raw.data)
    assert raw[:GUARD_BAND + 3] == bytes([GUARD_FILL]) * (GUARD_BAND + 3)
    assert raw[GUARD_BAND + 3 + 21:] == bytes([GUARD_FILL]) * GUARD_BAND and len(raw) == 2 * GUARD_BAND + 3 + 21
    g.memset(GUARD_FILL)          # a payload that happens to hold the fill byte is no finding
    g.memset(0x11, 4, 2)
    g.check("ah_anything")
    assert bytes(g._raw.data)[GUARD_BAND + 3 + 2:GUARD_BAND + 3 + 6] == b"\x11" * 4
    for bad in (lambda: g.upload(np.zeros(22, np.uint8)), lambda: g.download(np.uint8, 22), lambda: g.memset(0, 2, 20),
                lambda: g.download(np.uint8, 1, -1)):
        with pytest.raises(AssertionError):   # the payload's accessors never reach a band
            bad()


def test_guard_lead_gives_the_phase_asked_for():
    ctx = _HostCtx()
    for lead in range(0, 33):
        g = GuardedBuffer(ctx, 64, lead)
        assert g.base % 256 == 0 and g.ptr % 16 == lead % 16 and g.ptr - g.base == GUARD_BAND + lead


def test_guard_free_releases_the_base_pointer():
    ctx = _HostCtx()
    g = GuardedBuffer(ctx, 100, 7)
    base = g.base
    assert base == ctx.bufs[0].ptr and g.ptr != base
    g.free()
    assert ctx.freed == [base] and g.ptr == 0
    g.free()                      # twice is harmless
    assert ctx.freed == [base]


def test_guard_is_a_device_buffer():
    from arrow_go_amd.device import DeviceBuffer, _ptr
    g = GuardedBuffer(_HostCtx(), 8, 4)
    assert isinstance(g, DeviceBuffer) and _ptr(g) == g.ptr


def test_no_padded_output_is_left_in_the_backend():
    """every HipBackend output goes through _out(): the spare bytes of the old harness (`_dirty(n * w + 64)` / `+ 128`) are gone"""
    text = open(os.path.join(ROOT, "tests", "backends.py")).read()
    assert not re.findall(r"_dirty\([^)\n]*\+ *(?:64|128)\)", text)
    hipb = text[text.index("class HipBackend"):]
    assert len(re.findall(r"self\.c\.alloc\(", hipb)) == 2      # _dirty and _up: inputs only


def test_the_tiles_are_the_kernels_tiles():
    src = lambda f: open(os.path.join(CSRC, f)).read()
    num = lambda f, pat: int(re.search(pat, src(f)).group(1))
    assert num("ah_filter.hip", r"#define AH_FILTER_TILE_BYTES (\d+)") == FILTER_TILE_BYTES
    assert num("ah_take.hip", r"constexpr int kBlock = (\d+);") * num("ah_take.hip", r"#define AH_TAKE_UNROLL (\d+)") == TAKE_TILE
    assert num("ah_varlen.hip", r"constexpr int kBlock = (\d+);") == VARLEN_TILE
    assert num("ah_sort_radix.h", r"constexpr int kBlock = (\d+);") * num("ah_sort_radix.h", r"constexpr int kItems = (\d+);") == SORT_TILE
    assert re.search(r"constexpr int kTile = kBlock \* kItems;", src("ah_sort_radix.h"))
    assert num("ah_hash.hip", r"constexpr int kSmallBlock = (\d+);") * num("ah_hash.hip", r"constexpr int kSmallRows = (\d+);") == HASH_TILE
    assert num("ah_cast_impl.h", r"constexpr int kBlock = (\d+);") == BOOL_CAST_BLOCK
    scan = src("ah_scan.hip")
    assert num("ah_scan.hip", r"constexpr int kBlock = (\d+);") == 256
    assert "static constexpr int WCHUNK = 64 * VPT * V;" in scan and "static constexpr int TILE = (kBlock / 64) * WCHUNK;" in scan
    assert "(sizeof(T) >= 4 ? 8 : 4)" in scan
    assert scan.count("n >= ((int64_t)1 << 18)") == 3 and SCAN_ONEPASS_ROWS == 1 << 18
    assert [scan_tile(w) for w in (1, 2, 4, 8)] == [16384, 8192, 8192, 4096]
    ctxs = src("ah_ctx.hip")
    assert "nbytes >= ((size_t)1 << 20) && ((d | s) & 15) == 0 && disjoint" in ctxs      # ah_copy_async's vector path


# ---- on the GPU -------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@gpu
def test_guard_on_a_device_buffer(ctx):
    """the same one-byte cases on a real allocation: the stray byte is a one-byte memset inside the allocation"""
    _check_guard_reports(ctx, lambda raw, at: raw.memset(0x00, 1, at))
    for lead in (0, 1, 8, 15, 20):
        g = GuardedBuffer(ctx, 64, lead)
        assert g.base % 256 == 0 and g.ptr % 16 == lead % 16
        g.free()
        assert g.ptr == 0


@gpu
def test_backend_reports_an_entry_point_that_writes_outside(ctx):
    """HipBackend._run names the entry point and the output when a band changes, after success and after an error status"""
    import arrow_go_amd as ah
    be = HipBackend(ctx)
    ob = be._out("out_values", 24, 8)

    def stray():
        ob._raw.memset(0x00, 1, GUARD_BAND + 8 + 24 + 2)
    with pytest.raises(AssertionError, match=r"ah_entry: wrote outside out_values \(24 bytes at phase 8\): back band changed, nearest byte 3 "):
        be._run("ah_entry", stray)
    assert be._guards == []
    ob = be._out("out", 16)

    def stray_then_fail():
        ob._raw.memset(0x00, 1, GUARD_BAND - 16)
        raise ah.ErrOverflow("overflow")
    with pytest.raises(AssertionError, match=r"ah_failing: wrote outside out .*front band changed, nearest byte 16 "):
        be._run("ah_failing", stray_then_fail)
    ob = be._out("out", 16)

    def fail():
        raise ah.ErrOverflow("overflow")
    with pytest.raises(ah.ErrOverflow):          # a clean failure stays the failure it was
        be._run("ah_failing", fail)


def lengths(V):
    """around one vector, one wave of vectors, one block iteration of 256 lanes × 4 vectors"""
    out = []
    for n in [0, 1, V - 1, V, V + 1, 2 * V + 1, 64 * V - 1, 64 * V + 1, 1024 * V - 1, 1024 * V, 1024 * V + V + 1]:
        if n not in out:
            out.append(n)
    return out


def tile_rows(tile, V):
    return [1, V + 1, tile - 1, tile, tile + 1]


def phases(w):
    return list(range(0, 16, w))


def two_inputs(k, out_phase, w):
    """element shifts of the left and the right input, rotated over the cases: both on a line, one element off on either side alone,
    and all three operands on the output's non-zero phase (both inputs one element off when the output is on a line)"""
    c = k % 4
    if c < 3:
        return [(0, 0), (1, 0), (0, 1)][c]
    m = out_phase // w if out_phase else 1
    return m, m


def one_input(k, out_phase, w_in):
    """element shift of the one input: on a line, one element off, on the output's phase"""
    c = k % 3
    if c < 2:
        return c
    return out_phase // w_in if out_phase and out_phase % w_in == 0 else 1


EW_DTYPES = OL.ALL_DTYPES      # every width, signed, unsigned and floating
EW_INTS = OL.INT_DTYPES


# ---- 1. element-wise values -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", EW_DTYPES, ids=str)
def test_arithmetic_phases(hip, orc_be, dtype):
    w = np.dtype(dtype).itemsize
    rng = np.random.default_rng(7100 + w)
    for li, n in enumerate(lengths(16 // w)):
        l, r, s = rand(rng, dtype, n), rand(rng, dtype, n), rand(rng, dtype, 1)
        cases = [(ADD, AA, l, r), (ADD, AS, l, s), (ADD, SA, s, r), (SUB, AA, l, r), (MUL, AA, l, r)]
        exp = [orc_be.arithmetic(op, shape, a, b) for op, shape, a, b in cases]
        for pj, p in enumerate(phases(w)):
            ml, mr = two_inputs(li + pj, p, w)
            for (op, shape, a, b), e in zip(cases, exp):
                g = hip.arithmetic(op, shape, a, b, misalign_l=ml, misalign_r=mr, out_phase=p)
                assert same_bits_or_both_nan(g, e), (dtype, op, shape, n, p, ml, mr)


@gpu
@pytest.mark.parametrize("dtype", EW_DTYPES, ids=str)
def test_unary_phases(hip, orc_be, dtype):
    w = np.dtype(dtype).itemsize
    rng = np.random.default_rng(7200 + w)
    for li, n in enumerate(lengths(16 // w)):
        a = rand(rng, dtype, n)
        exp = [orc_be.arithmetic_unary(op, a) for op in (4, 5, 20)]
        for pj, p in enumerate(phases(w)):
            mi = one_input(li + pj, p, w)
            for op, e in zip((4, 5, 20), exp):
                assert hip.arithmetic_unary(op, a, misalign_in=mi, out_phase=p).tobytes() == e.tobytes(), (dtype, op, n, p, mi)


@gpu
@pytest.mark.parametrize("dtype", EW_INTS, ids=str)
def test_checked_phases(hip, orc_be, dtype):
    """nulls on both sides; small operands (nothing overflows: every byte, zeros under nulls) and full-range ones (the verdict — a
    failed call is checked for its extents like a successful one)"""
    w = np.dtype(dtype).itemsize
    rng = np.random.default_rng(7300 + w)
    for li, n in enumerate(lengths(16 // w)):
        l, r = rng.integers(6, 11, n).astype(dtype), rng.integers(0, 6, n).astype(dtype)
        L, R = rand(rng, dtype, n), rand(rng, dtype, n)
        lv, rv = rand_bits(rng, n + 5, 0.8), rand_bits(rng, n + 9, 0.8)
        exp = [orc_be.arithmetic_checked(op, AA, l, lv, 5, r, rv, 9) for op in (21, 22, 23)]
        exp_wide = orc_be.arithmetic_checked(21, AA, L, lv, 5, R, rv, 9)
        for pj, p in enumerate(phases(w)):
            ml, mr = two_inputs(li + pj, p, w)
            for op, (st_o, out_o) in zip((21, 22, 23), exp):
                st_h, out_h = hip.arithmetic_checked(op, AA, l, lv, 5, r, rv, 9, misalign_l=ml, misalign_r=mr, out_phase=p)
                assert st_h == st_o == STATUS_OK and out_h.tobytes() == out_o.tobytes(), (dtype, op, n, p, ml, mr)
            st_h, out_h = hip.arithmetic_checked(21, AA, L, lv, 5, R, rv, 9, misalign_l=ml, misalign_r=mr, out_phase=p)
            assert st_h == exp_wide[0], (dtype, n, p)
            if st_h == STATUS_OK:
                assert out_h.tobytes() == exp_wide[1].tobytes(), (dtype, n, p)


@gpu
@pytest.mark.parametrize("dtype", EW_DTYPES, ids=str)
def test_arithmetic_ext_phases(hip, orc_be, dtype):
    """DIV, SHIFT_LEFT, BIT_AND, NOT for the integers, DIV and SQRT for the floats; validity on both sides"""
    dt = np.dtype(dtype)
    w = dt.itemsize
    rng = np.random.default_rng(7400 + w)
    for li, n in enumerate(lengths(16 // w)):
        lv, rv = rand_bits(rng, n + 16, 0.85), rand_bits(rng, n + 16, 0.85)
        if dt.kind == "f":
            a = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(dtype)
            b = (rng.standard_normal(n) * 10.0 ** rng.integers(-30, 30, n)).astype(dtype)
            cases = [(_XOPS["DIV"], 0, a, lv, 3, b, rv, 5), (_XOPS["SQRT"], 1, a, lv, 3, None, None, 0)]
        else:
            info = np.iinfo(dtype)
            a, b = rand(rng, dtype, n), rand(rng, dtype, n)
            b[b == 0] = 1
            counts = rng.integers(0, info.bits - 1, n).astype(dtype)
            cases = [(_XOPS["DIV"], 0, a, lv, 3, b, rv, 5), (_XOPS["SHL"], 0, a, lv, 3, counts, rv, 5), (_XOPS["AND"], 0, a, lv, 3, b, rv, 5),
                     (_XOPS["NOT"], 1, a, lv, 3, None, None, 0)]
        with np.errstate(all="ignore"):
            exp = [orc_be.arithmetic_ext(*c) for c in cases]
        for pj, p in enumerate(phases(w)):
            ml, mr = two_inputs(li + pj, p, w)
            for c, e in zip(cases, exp):
                _ext_same(hip.arithmetic_ext(*c, misalign_l=ml, misalign_r=mr, out_phase=p), e, (dtype, c[0], n, p, ml, mr))


@gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=str)
def test_round_phases(hip, orc_be, dtype):
    w = np.dtype(dtype).itemsize
    rng = np.random.default_rng(7500 + w)
    for li, n in enumerate(lengths(16 // w)):
        x = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 6, n)).astype(dtype)
        valid = rand_bits(rng, n + 8, 0.9)
        mode = li % 10
        exp = [orc_be.round(x, valid, 3, 2, mode), orc_be.round(x, None, 0, -1, mode), orc_be.round(x, valid, 3, 0, mode, multiple=0.25)]
        for pj, p in enumerate(phases(w)):
            mi = one_input(li + pj, p, w)
            got = [hip.round(x, valid, 3, 2, mode, misalign_in=mi, out_phase=p), hip.round(x, None, 0, -1, mode, misalign_in=mi, out_phase=p),
                   hip.round(x, valid, 3, 0, mode, multiple=0.25, misalign_in=mi, out_phase=p)]
            for g, e in zip(got, exp):
                assert g[0] == e[0] == 0 and g[1].tobytes() == e[1].tobytes(), (dtype, n, p, mi, mode)


@gpu
@pytest.mark.parametrize("in_t,out_t", [(np.int32, np.int32), (np.int32, np.int64), (np.int64, np.int32), (np.int64, np.int64)],
                         ids=["32to32", "32to64", "64to32", "64to64"])
def test_shift_time_phases(hip, orc_be, in_t, out_t):
    wi, wo = np.dtype(in_t).itemsize, np.dtype(out_t).itemsize
    rng = np.random.default_rng(7600 + 10 * wi + wo)
    info = np.iinfo(in_t)
    for li, n in enumerate(lengths(16 // wo)):
        wide = rng.integers(info.min, info.max, n, dtype=in_t, endpoint=True)
        small = (rng.integers(-1000, 1000, n) * 1000).astype(in_t)
        valid = OL.pack_bits(rng.random(n + 5) < 0.8)
        calls = [(wide, out_t, 0, 1000, False, valid, 5), (wide, out_t, 1, 1000, False, valid, 5), (small, out_t, 0, 1000, True, valid, 5),
                 (wide, out_t, 0, 86400000, True, valid, 5)]
        exp = [orc_be.shift_time(*c) for c in calls]
        for pj, p in enumerate(phases(wo)):
            mi = one_input(li + pj, p, wi)
            for c, (st_e, e, bad_e) in zip(calls, exp):
                st_g, g, bad_g = hip.shift_time(*c, misalign_in=mi, out_phase=p)
                assert st_g == st_e, (n, p, mi, c[2:5])
                if st_e == STATUS_OK:
                    assert g.tobytes() == e.tobytes(), (n, p, mi, c[2:5])
                else:
                    assert bad_g == bad_e, (n, p, mi, c[2:5])


# per input width: one narrowing, one widening and one float <-> int cast (a 1-byte input cannot narrow, an 8-byte one cannot widen)
CAST_PAIRS = [(np.uint8, np.int32), (np.uint8, np.float32),
              (np.int16, np.int8), (np.int16, np.int64), (np.int16, np.float64),
              (np.int32, np.int16), (np.int32, np.int64), (np.float32, np.int32),
              (np.int64, np.uint8), (np.float64, np.int64), (np.int64, np.float32)]


@gpu
@pytest.mark.parametrize("frm,to", CAST_PAIRS, ids=lambda t: np.dtype(t).name)
def test_cast_numeric_phases(hip, orc_be, frm, to):
    """unchecked (every slot converted) and safe (the verdict; the values when it passes) casts"""
    wi, wo = np.dtype(frm).itemsize, np.dtype(to).itemsize
    rng = np.random.default_rng(7700 + 10 * wi + wo)
    for li, n in enumerate(lengths(16 // wo)):
        a = cast_input(rng, frm, to, n, in_range=False)
        ok_in = cast_input(rng, frm, to, n, in_range=True)
        with np.errstate(all="ignore"):
            e_un, e_ok, e_bad = orc_be.cast_numeric(a, to, None, 0, True, True), orc_be.cast_numeric(ok_in, to), orc_be.cast_numeric(a, to)
        assert e_un[0] == e_ok[0] == STATUS_OK
        for pj, p in enumerate(phases(wo)):
            mi = one_input(li + pj, p, wi)
            st, g, _ = hip.cast_numeric(a, to, None, 0, True, True, misalign_in=mi, out_phase=p)
            assert st == STATUS_OK and same_bits_or_both_nan(g, e_un[1]), (frm, to, n, p, mi)
            st, g, _ = hip.cast_numeric(ok_in, to, misalign_in=mi, out_phase=p)
            assert st == STATUS_OK and g.tobytes() == e_ok[1].tobytes(), (frm, to, n, p, mi)
            st, g, _ = hip.cast_numeric(a, to, misalign_in=mi, out_phase=p)
            assert st == e_bad[0], (frm, to, n, p, mi)
            if st == STATUS_OK:
                assert same_bits_or_both_nan(g, e_bad[1]), (frm, to, n, p, mi)


# ---- 2. compacting and gathering outputs ------------------------------------------------------------------------------------------------
SEL_P = 0.37    # leaves a ragged n_out at every row count below


@gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.float32, np.int64], ids=str)
def test_filter_phases(hip, orc_be, dtype):
    """ah_filter_primitive, _once (both inside HipBackend.filter) and _dev; DROP and EMIT, with and without validity"""
    w = np.dtype(dtype).itemsize
    rng = np.random.default_rng(7800 + w)
    for li, n in enumerate(tile_rows(FILTER_TILE_BYTES // w, 16 // w)):
        vals = rand(rng, dtype, n)
        fdata = rand_bits(rng, n + 80, SEL_P)
        for vvalid, fvalid, voff, foff in [(None, None, 0, 0), (rand_bits(rng, n + 80, 0.9), rand_bits(rng, n + 80, 0.9), 3, 9)]:
            want_valid = vvalid is not None
            for null_sel in (DROP, EMIT):
                e = orc_be.filter(vals, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid)
                for pj, p in enumerate(phases(w)):
                    mv = (li + pj) % 3
                    for flavour in (hip.filter, hip.filter_dev):
                        g = flavour(vals, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid, misalign=mv, out_phase=p)
                        assert g[0].tobytes() == e[0].tobytes(), (dtype, n, null_sel, p, mv, flavour.__name__)
                        if want_valid:
                            assert g[1].tobytes() == e[1].tobytes(), (dtype, n, null_sel, p, mv, flavour.__name__)
                        assert g[2] == e[2]


@gpu
def test_filter_to_indices_phases(hip, orc_be):
    rng = np.random.default_rng(7900)
    for n in tile_rows(FILTER_TILE_BYTES // 4, 4):
        fdata, fvalid = rand_bits(rng, n + 80, SEL_P), rand_bits(rng, n + 80, 0.9)
        for foff in (0, 11):
            for fv in (None, fvalid):
                for null_sel in (DROP, EMIT):
                    want_valid = fv is not None and null_sel == EMIT
                    e = orc_be.filter_to_indices(fdata, fv, foff, n, null_sel, want_valid)
                    for p in phases(4):
                        g = hip.filter_to_indices(fdata, fv, foff, n, null_sel, want_valid, out_phase=p)
                        assert g[0].tobytes() == e[0].tobytes(), (n, foff, null_sel, p)
                        if want_valid:
                            assert g[1].tobytes() == e[1].tobytes() and g[2] == e[2], (n, foff, null_sel, p)


def _take_sweep(hip, orc_be, rng, vals, w, idtypes, rows):
    nvalues = vals.size
    for li, nidx in enumerate(rows):
        idtype = idtypes[li % len(idtypes)]
        idx = rng.integers(0, min(nvalues, np.iinfo(idtype).max + 1), nidx).astype(idtype)
        for vvalid, ivalid, voff, ioff in [(None, None, 0, 0), (rand_bits(rng, 5 + nvalues + 8, 0.9), rand_bits(rng, 3 + nidx + 8, 0.9), 5, 3)]:
            want_valid = vvalid is not None
            e = orc_be.take(vals, vvalid, voff, idx, ivalid, ioff, True, want_valid)
            for pj, p in enumerate(phases(w)):
                mv, mi = (li + pj) % 3, (li + pj + 1) % 2
                g = hip.take(vals, vvalid, voff, idx, ivalid, ioff, True, want_valid, misalign_values=mv, misalign_idx=mi, out_phase=p)
                assert g[0] == e[0] == STATUS_OK and g[1].tobytes() == e[1].tobytes(), (w, idtype, nidx, p, mv, mi)
                if want_valid:
                    assert g[2].tobytes() == e[2].tobytes() and g[3] == e[3], (w, idtype, nidx, p)
                d = hip.take_dev(vals, vvalid, voff, idx, ivalid, ioff, want_valid, misalign_values=mv, misalign_idx=mi, out_phase=p)
                assert d[3] is None and d[0].tobytes() == e[1].tobytes(), (w, idtype, nidx, p, mv, mi)
                if want_valid:
                    assert d[1].tobytes() == e[2].tobytes() and d[2] == e[3], (w, idtype, nidx, p)


@gpu
@pytest.mark.parametrize("vdtype", [np.uint8, np.int16, np.float32, np.int64], ids=str)
def test_take_phases(hip, orc_be, vdtype):
    """ah_take_primitive and _dev: values, indices and output each on a phase of their own; every index width in turn"""
    w = np.dtype(vdtype).itemsize
    rng = np.random.default_rng(8000 + w)
    _take_sweep(hip, orc_be, rng, rand(rng, vdtype, 300), w, [np.int32, np.int64, np.uint16, np.int8, np.uint32], tile_rows(TAKE_TILE, 16 // w))


@gpu
@pytest.mark.parametrize("w", [16, 3])
def test_take_wide_slot_phases(hip, orc_be, w):
    """FSBImpl's slots: 16 bytes (one vector per row) and 3 bytes (the byte-wise kernel: six phases of a line)"""
    rng = np.random.default_rng(8100 + w)
    vals = rng.integers(0, 256, (300, w), dtype=np.uint8).view(np.dtype(f"V{w}")).reshape(-1)
    _take_sweep(hip, orc_be, rng, vals, w, [np.int32, np.int64, np.uint16], tile_rows(TAKE_TILE, max(16 // w, 1)))


@gpu
@pytest.mark.parametrize("odt", [np.int32, np.int64], ids=["binary", "large_binary"])
def test_take_binary_phases(hip, orc_be, odt):
    """ah_take_binary_offsets / _data: the output offsets on every phase of their width, the output bytes on a phase that walks the line"""
    w = np.dtype(odt).itemsize
    rng = np.random.default_rng(8200 + w)
    nvals = 200
    offsets, data, vvalid = random_binary(rng, nvals, odt, 7, 0.15)
    for li, n in enumerate(tile_rows(VARLEN_TILE, 16 // w)):
        idx = rng.integers(0, nvals, n).astype(np.int32)
        ivalid = OL.pack_bits(list(rng.random(n) >= 0.1))
        for vv, iv in [(None, None), (vvalid, ivalid)]:
            want_valid = vv is not None
            e = orc_be.take_binary(offsets, data, vv, 0, nvals, idx, iv, 0, want_valid)
            for pj, p in enumerate(phases(w)):
                k = li + pj
                g = hip.take_binary(offsets, data, vv, 0, nvals, idx, iv, 0, want_valid, misalign_offsets=k % 2, misalign_data=k % 5,
                                    misalign_idx=(k + 1) % 2, out_phase=p, data_phase=(5 * k + 1) % 16)
                assert e[0] == g[0] == STATUS_OK
                assert g[1].tobytes() == e[1].tobytes() and g[2].tobytes() == e[2].tobytes(), (odt, n, p, k)
                if want_valid:
                    assert g[3].tobytes() == e[3].tobytes() and g[4] == e[4], (odt, n, p, k)


def _cumsum_same(g, e, n, what):
    assert g[0] == e[0], what
    if e[0] == STATUS_OK:
        assert g[1].tobytes() == e[1].tobytes(), what
        if e[2] is not None:
            bits = lambda b: np.unpackbits(np.asarray(b, np.uint8), bitorder="little")[:n]
            assert (bits(g[2]) == bits(e[2])).all() and g[3] == e[3], what


@gpu
@pytest.mark.parametrize("dtype", OL.INT_DTYPES, ids=str)
def test_cumulative_sum_phases(hip, orc_be, dtype):
    """plain, checked and with nulls, around one tile of the reduce-then-scan kernels and — for the widths that have one-pass kernels
    — around the row count from which a 16-byte aligned call takes them (every other phase stays on reduce-then-scan there)"""
    w = np.dtype(dtype).itemsize
    rng = np.random.default_rng(8300 + w)
    rows = tile_rows(scan_tile(w), 16 // w)
    if w >= 2:
        rows += [SCAN_ONEPASS_ROWS - 1, SCAN_ONEPASS_ROWS, SCAN_ONEPASS_ROWS + 1]
    for li, n in enumerate(rows):
        vals = (rng.random(n) < 0.001).astype(dtype) if n > 1000 else rng.integers(0, 5, n).astype(dtype)   # (no overflow in 2 bytes either)
        wide = rand(rng, dtype, n)
        valid = rand_bits(rng, n + 8, 0.9)
        calls = [(wide, None, 0, None, False, False), (vals, None, 0, np.dtype(dtype).type(3), False, True), (vals, valid, 3, None, True, True),
                 (wide, valid, 3, None, False, False)]
        exp = [orc_be.cumulative_sum(*c) for c in calls]
        for pj, p in enumerate(phases(w)):
            mi = one_input(li + pj, p, w) if p or n < SCAN_ONEPASS_ROWS - 1 else 0      # (phase 0 at the threshold: both on a line)
            for c, e in zip(calls, exp):
                _cumsum_same(hip.cumulative_sum(*c, misalign_in=mi, out_phase=p), e, n, (dtype, n, p, mi, c[3:]))


@gpu
@pytest.mark.parametrize("out_t", OL.ALL_DTYPES, ids=str)
def test_cast_bool_to_numeric_phases(hip, orc_be, out_t):
    w = np.dtype(out_t).itemsize
    rng = np.random.default_rng(8400 + w)
    for n in tile_rows(BOOL_CAST_BLOCK * (16 // w), 16 // w):
        for off in (0, 13):
            bits = OL.pack_bits(list(rng.random(off + n) < 0.5))
            e = orc_be.cast_bool_to_numeric(bits, off, n, out_t)
            for p in phases(w):
                assert hip.cast_bool_to_numeric(bits, off, n, out_t, out_phase=p).tobytes() == e.tobytes(), (out_t, n, off, p)


@gpu
@pytest.mark.parametrize("dtype", OL.ALL_DTYPES, ids=str)
def test_sort_indices_phases(hip, orc_be, dtype):
    rng = np.random.default_rng(8500 + np.dtype(dtype).itemsize)
    for li, n in enumerate(tile_rows(SORT_TILE, 2)):
        vals = rand(rng, dtype, n, small=li % 2 == 0)     # ties everywhere / full range (NaN, ±inf, -0.0 for the floats)
        valid = rand_bits(rng, n + 8, 0.9)
        for v, off, desc, nfirst in [(None, 0, False, False), (valid, 3, True, True)]:
            e = orc_be.sort_indices(vals, v, off, desc, nfirst)
            for pj, p in enumerate(phases(8)):
                g = hip.sort_indices(vals, v, off, desc, nfirst, misalign=(li + pj) % 2, out_phase=p)
                assert g.tobytes() == e.tobytes(), (dtype, n, desc, p)
                if v is None and not desc:
                    g = hip.sort_indices_multi([(vals, None, 0, False, False), (vals[::-1].copy(), None, 0, True, False)], out_phase=p)
                    assert g.tobytes() == orc_be.sort_indices_multi([(vals, None, 0, False, False), (vals[::-1].copy(), None, 0, True, False)]).tobytes()


@gpu
def test_hash_encode_phases(hip, orc_be):
    """ah_hash_u64_encode: the ids on every phase of their width, the dictionary on both of its own, the keys shifted on their own"""
    rng = np.random.default_rng(8600)
    for li, n in enumerate(tile_rows(HASH_TILE, 4)):
        keys = (rng.integers(0, 97, n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
        valid = rand_bits(rng, n + 8, 0.9)
        for v, off, enc in [(None, 0, False), (valid, 3, True), (valid, 3, False)]:
            e = orc_be.hash_encode(keys, v, off, enc)
            for pj, p in enumerate(phases(4)):
                k = li + pj
                g = hip.hash_encode(keys, v, off, enc, misalign_keys=k % 2, out_phase=p, dict_phase=8 * ((k // 2) % 2))
                assert g[0].tobytes() == e[0].tobytes() and g[2].tobytes() == e[2].tobytes() and g[3] == e[3], (n, enc, p, k)
                if v is not None and not enc:
                    assert g[1].tobytes() == e[1].tobytes(), (n, p)


# ---- 3. ah_copy_async -------------------------------------------------------------------------------------------------------------------
@gpu
def test_copy_async_phases(hip):
    """the 16-byte-per-lane kernel starts at 1 MiB on 16-byte aligned ranges; every other phase and the tail behind the last whole
    vector go through the runtime's copy: the destination holds the source's bytes and nothing around it changes"""
    mib = 1 << 20
    src = np.random.default_rng(8700).integers(0, 256, mib + 17, dtype=np.uint8)
    for nbytes in (mib - 1, mib, mib + 1, mib + 17):
        for dp in (0, 1, 8, 15):
            for sp in (0, 3):
                got = hip.copy(src[:nbytes], src_phase=sp, dst_phase=dp)
                assert got.tobytes() == src[:nbytes].tobytes(), (nbytes, dp, sp)
