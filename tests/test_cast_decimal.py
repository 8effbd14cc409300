"""Decimal casts through `cast`: Decimal128 / 256 → Decimal128 / 256 (rescale, precision, width), the 8 integer types → decimal,
decimal → the 8 integer types (CastDecimalToDecimal, CastIntegerToDecimal, CastDecimal128ToInteger / CastDecimal256ToInteger:
arrow/compute/internal/kernels/numeric_cast.go:79-429; cast_decimal / cast_decimal256: compute/cast.go:883-885).

Expected values never come from the code under test:
  * `restate_*` below: the rules in Python integers — compared over VALUE BYTES OF EVERY SLOT (zeros under nulls), validity and null count;
  * the reference's own tables (compute/cast_test.go:631-1255), transcribed;
  * pyarrow.compute.cast as a third opinion wherever Arrow C++ and the reference agree — everything except decimal → integer with
    allow_decimal_truncate on rows whose dropped fraction is ≥ ½ in magnitude (the reference rounds half away from zero, Arrow C++
    truncates): those rows are checked by the restatement alone (`test_decimal_to_int_truncate_rounds_half_away_from_zero`) — and
    safe Decimal256 → uint64 of values in [2^63, 2^64), which pyarrow refuses wrongly (`test_random_integer_decimal_parity`).
    pyarrow is asked about each column with zeros under its nulls (Arrow C++ checks the payload of null slots)."""
import ctypes
import decimal
import os
import re
import subprocess
import tempfile

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow_go_amd", "csrc")
D = decimal.Decimal
INT_TYPES = [pa.uint8(), pa.int8(), pa.uint16(), pa.int16(), pa.uint32(), pa.int32(), pa.uint64(), pa.int64()]
INT_IDS = {pa.uint8(): 2, pa.int8(): 3, pa.uint16(): 4, pa.int16(): 5, pa.uint32(): 6, pa.int32(): 7, pa.uint64(): 8, pa.int64(): 9}
MAX_DIGITS = {8: 3, 16: 5, 32: 10}          # MaxDecimalDigitsForInt (kernels/helpers.go:705-719); 64 bits: 19 signed, 20 unsigned
LOSS, NOFIT, BOUNDS = "rescale data loss", "decimal value does not fit in precision", "integer value out of bounds"


def dec_type(width, p, s):
    return pa.decimal128(p, s) if width == 128 else pa.decimal256(p, s)


def fmt(t):
    """the option text of a target type"""
    if pa.types.is_decimal(t):
        return "d:%d,%d%s" % (t.precision, t.scale, ",256" if t.bit_width == 256 else "")
    return {"float": "float", "double": "double"}.get(str(t), str(t))


# ---- no GPU needed ------------------------------------------------------------------------------------------------------------------
def _dispatch(fn, tid):
    from arrow_go_amd import compute as ac
    tin, tout, err = (ctypes.c_int * 1)(tid), (ctypes.c_int * 1)(), ctypes.create_string_buffer(512)
    return ac.lib.ahc_dispatch_best(fn.encode(), 1, tin, tout, err, len(err)), err.value.decode()


def test_registry_has_the_decimal_cast_functions_and_kernels():
    from arrow_go_amd import compute as ac
    for fn in ("cast_decimal", "cast_decimal256"):
        assert ac.lib.ahc_has_function(fn.encode()), fn
        for tid in list(range(2, 10)) + [23, 24]:
            rc, err = _dispatch(fn, tid)
            assert rc == 0, (fn, tid, err)
        for tid in (1, 11, 12, 13, 14, 34):          # bool, float32, float64, utf8, binary, large_utf8: out of scope, refused
            rc, err = _dispatch(fn, tid)
            assert rc != 0 and "no kernel matching" in err, (fn, tid, err)
    for name in ("uint8", "int8", "uint16", "int16", "uint32", "int32", "uint64", "int64"):
        for tid in (23, 24):
            rc, err = _dispatch("cast_" + name, tid)
            assert rc == 0, (name, tid, err)
    for name in ("float", "double", "boolean"):      # float ↔ decimal and boolean ↔ decimal: out of scope
        for tid in (23, 24):
            assert _dispatch("cast_" + name, tid)[0] != 0, name


def test_decimal_cast_entry_points_are_declared_and_exported():
    from arrow_go_amd import _native as N
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for sym in ("ah_cast_decimal_rescale", "ah_cast_int_to_decimal", "ah_cast_decimal_to_int"):
        assert sym in N.declared_symbols() and sym in exported, sym


def test_decimal_cast_kernels_have_no_scratch_and_move_sixteen_bytes():
    """every kernel of ah_cast_decimal.hip compiles for gfx950 with zero scratch bytes (read from the ISA, as tests/test_isa_hints.py
    reads it), loads decimals 16 bytes at a time and stores them so; the comparisons' kernel keeps its register budget with the
    shared header (tests/test_isa_hints.py holds that bar)"""
    import shutil
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "cast_decimal.s")
        r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-S",
                            "--cuda-device-only", "-o", out, os.path.join(CSRC, "ah_cast_decimal.hip")], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(out).read()
    kernels = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        v = re.search(r"\.amdhsa_next_free_vgpr (\d+)", m.group(2))
        p = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
        kernels[m.group(1)] = (int(v.group(1)), int(p.group(1)))
    assert sum("rescale_kernel" in k for k in kernels) == 30
    assert sum("int_to_decimal_kernel" in k for k in kernels) == 16
    assert sum("decimal_to_int_kernel" in k for k in kernels) == 24
    for k, (vgpr, scratch) in kernels.items():
        assert scratch == 0, f"{k}: {scratch} bytes of scratch ({vgpr} VGPRs)"
    assert "scratch_" not in text
    body = {}
    cur = None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            body[cur] = []
        elif cur and line.startswith(".Lfunc_end"):
            cur = None
        elif cur:
            body[cur].append(line)
    for k, lines in body.items():
        ins = " ".join(lines)
        if "rescale_kernel" in k or "decimal_to_int_kernel" in k:
            assert "global_load_dwordx4" in ins, k
        if "rescale_kernel" in k or "int_to_decimal_kernel" in k:
            assert "global_store_dwordx4" in ins, k


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def to_signed(v, bits):
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def trunc_div(v, d):
    q = abs(v) // d
    return -q if v < 0 else q


def restate_rescale(slots, valid, in_scale, out_t, allow_truncate, in_bits):
    """decimal → decimal: (unscaled output integer of every slot, error text of the first offending valid row or None)"""
    k = out_t.scale - in_scale
    out = []
    for v, ok in zip(slots, valid):
        if not ok:
            out.append(0)
            continue
        if allow_truncate:
            r = v * 10 ** k if k > 0 else trunc_div(v, 10 ** -k)
            out.append(to_signed(r, out_t.bit_width))          # × wraps modulo 2^bits; 256 → 128 keeps the low 128 bits
            continue
        if k >= 0:
            r = v * 10 ** k
        else:
            if abs(v) % 10 ** -k:
                return None, LOSS
            r = trunc_div(v, 10 ** -k)
        if abs(r) >= 10 ** out_t.precision:
            return None, NOFIT
        out.append(r)
    return out, None


def restate_int_to_decimal(slots, valid, out_t):
    return [v * 10 ** out_t.scale if ok else 0 for v, ok in zip(slots, valid)]


def restate_decimal_to_int(slots, valid, in_scale, out_t, allow_truncate, allow_overflow):
    bits = out_t.bit_width
    signed = pa.types.is_signed_integer(out_t)
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    out = []
    for v, ok in zip(slots, valid):
        if not ok:
            out.append(0)
            continue
        if in_scale < 0:
            r = v * 10 ** -in_scale
        elif in_scale == 0:
            r = v
        else:
            d = 10 ** in_scale
            q, rem = abs(v) // d, abs(v) % d
            if not allow_truncate:
                if rem:
                    return None, LOSS
            elif 2 * rem >= d:
                q += 1                                   # ReduceScaleBy(scale, round = true): half away from zero
            r = -q if v < 0 else q
        if not allow_overflow and not lo <= r <= hi:
            return None, BOUNDS
        r64 = to_signed(r, 64)                           # the low 64 bits, narrowed to the target
        out.append(to_signed(r64, bits) if signed else r64 & ((1 << bits) - 1))
    return out, None


# ---- building inputs and reading results ----------------------------------------------------------------------------------------------
def make_array(typ, slots, valid, offset=0, pad=0):
    """an array of `typ` whose buffers hold exactly `slots` (payloads under nulls and values beyond the declared precision included),
    behind `pad` leading slots of garbage when sliced at `offset`"""
    n = len(slots)
    if pa.types.is_decimal(typ):
        w = typ.byte_width
        raw = b"".join((s & ((1 << (8 * w)) - 1)).to_bytes(w, "little") for s in slots)
        data = b"\xEE" * (w * offset) + raw
    else:
        npdt = np.dtype(typ.to_pandas_dtype())
        data = np.concatenate([np.full(offset, 0x5A, npdt), np.array([s & ((1 << typ.bit_width) - 1) for s in slots], dtype=np.uint64).astype(npdt)]).tobytes()
    bits = np.zeros(offset + n, np.uint8)
    bits[offset:] = np.asarray(valid, np.uint8)
    bits[:offset] = 1
    vbuf = None if all(valid) and offset == 0 else pa.py_buffer(np.packbits(bits, bitorder="little").tobytes())
    return pa.Array.from_buffers(typ, n, [vbuf, pa.py_buffer(data)], null_count=int(n - sum(valid)), offset=offset)


def slots_of(arr):
    """(unscaled integer of every slot, validity list, null count) of a result — null slots read like the others"""
    t = arr.type
    n = len(arr)
    bufs = arr.buffers()
    w = t.byte_width if pa.types.is_decimal(t) else t.bit_width // 8
    data = bufs[1].to_pybytes()[arr.offset * w:(arr.offset + n) * w] if n else b""
    signed = pa.types.is_decimal(t) or pa.types.is_signed_integer(t)
    vals = [int.from_bytes(data[i * w:(i + 1) * w], "little", signed=signed) for i in range(n)]
    if bufs[0] is None:
        valid = [True] * n
    else:
        bits = np.unpackbits(np.frombuffer(bufs[0], np.uint8), bitorder="little")[arr.offset:arr.offset + n]
        valid = [bool(b) for b in bits]
    return vals, valid, arr.null_count


def opt_text(to, allow_truncate=False, allow_overflow=False):
    return "to_type=%s;allow_decimal_truncate=%d;allow_int_overflow=%d" % (fmt(to), int(allow_truncate), int(allow_overflow))


def check_cast(sess, arr, slots, valid, to, allow_truncate=False, allow_overflow=False, against_pyarrow=True):
    """cast through the session against the restatement (and pyarrow); returns the error text or None"""
    frm = arr.type
    if pa.types.is_decimal(frm) and pa.types.is_decimal(to):
        exp, err = restate_rescale(slots, valid, frm.scale, to, allow_truncate, frm.bit_width)
    elif pa.types.is_decimal(to):
        exp, err = restate_int_to_decimal(slots, valid, to), None
    else:
        exp, err = restate_decimal_to_int(slots, valid, frm.scale, to, allow_truncate, allow_overflow)
    opts = opt_text(to, allow_truncate, allow_overflow)
    # pyarrow's opinion is asked about the same column with zeros under its nulls: Arrow C++ looks at the payload of null slots
    ref_arr = make_array(frm, [v if ok else 0 for v, ok in zip(slots, valid)], valid, arr.offset) if against_pyarrow else None
    if err is not None:
        with pytest.raises(Exception, match=err):
            sess.call_function("cast", [arr], opts)
        if against_pyarrow:
            with pytest.raises(pa.ArrowInvalid):
                pc.cast(ref_arr, options=pc.CastOptions(to, allow_decimal_truncate=allow_truncate, allow_int_overflow=allow_overflow))
        return err
    got = sess.call_function("cast", [arr], opts)
    assert got.type == to, (got.type, to)
    g_vals, g_valid, g_nulls = slots_of(got)
    print("cast %s -> %s trunc=%d ovf=%d rows=%d mismatching slots=%d" % (frm, to, allow_truncate, allow_overflow, len(arr),
                                                                         sum(a != b for a, b in zip(g_vals, exp))))
    assert g_vals == exp, (frm, to, allow_truncate, allow_overflow)
    assert g_valid == list(map(bool, valid)) and g_nulls == len(valid) - sum(valid)
    if against_pyarrow:
        want = pc.cast(ref_arr, options=pc.CastOptions(to, allow_decimal_truncate=allow_truncate, allow_int_overflow=allow_overflow))
        assert got.to_pylist() == want.to_pylist(), (frm, to, allow_truncate, allow_overflow)
    return None


@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.close()


def dec_arr(width, p, s, texts):
    wide = decimal.Context(prec=100)
    vals = [None if t is None else D(t).quantize(D(1).scaleb(-s), context=wide) if s >= 0 else D(t) for t in texts]
    return pa.array(vals, dec_type(width, p, s))


def unscaled(arr):
    vals, valid, _ = slots_of(arr)
    return vals, valid


# ---- the reference's tables -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("width", [128, 256])
def test_reference_decimal_to_int_tables(sess, width):
    """TestDecimal128ToInt / TestDecimal256ToInt (compute/cast_test.go:631-752, 754-875)"""
    i64 = pa.int64()
    call = lambda a, trunc, ovf: sess.call_function("cast", [a], opt_text(i64, trunc, ovf))
    # no overflow no truncate: all four option combinations
    a = dec_arr(width, 38, 10, ["02.0000000000", "-11.0000000000", "22.0000000000", "-121.000000000", None])
    for ovf in (False, True):
        for trunc in (False, True):
            assert call(a, trunc, ovf).to_pylist() == [2, -11, 22, -121, None]
            check_cast(sess, a, *unscaled(a), i64, trunc, ovf)
    # truncate no overflow
    a = dec_arr(width, 38, 10, ["02.1000000000", "-11.0000004500", "22.0000004500", "-121.1210000000", None])
    for ovf in (False, True):
        assert call(a, True, ovf).to_pylist() == [2, -11, 22, -121, None]
        with pytest.raises(Exception, match=LOSS):
            call(a, False, ovf)
        check_cast(sess, a, *unscaled(a), i64, True, ovf)      # every dropped fraction is below ½: pyarrow agrees
    # overflow no truncate: the modulo-2^64 row
    a = dec_arr(width, 38, 10, ["12345678901234567890000.0000000000", "99999999999999999999999.0000000000", None])
    for trunc in (False, True):
        assert call(a, trunc, True).to_pylist() == [4807115922877858896, 200376420520689663, None]
        with pytest.raises(Exception, match=BOUNDS):
            call(a, trunc, False)
        check_cast(sess, a, *unscaled(a), i64, trunc, True)
    # overflow and truncate
    a = dec_arr(width, 38, 10, ["12345678901234567890000.0045345000", "99999999999999999999999.0000344300", None])
    for ovf in (False, True):
        for trunc in (False, True):
            if ovf and trunc:
                assert call(a, trunc, ovf).to_pylist() == [4807115922877858896, 200376420520689663, None]
            else:
                with pytest.raises(Exception):
                    call(a, trunc, ovf)
            check_cast(sess, a, *unscaled(a), i64, trunc, ovf, against_pyarrow=ovf and trunc)
    # negative scale: 1234567890000 and −120000 held at scale −4
    a = make_array(dec_type(width, 38, -4), [123456789, -12], [True, True])
    assert call(a, True, True).to_pylist() == [1234567890000, -120000]
    assert call(a, False, False).to_pylist() == [1234567890000, -120000]
    # int64 bounds inclusive, and one beyond
    a = dec_arr(width, 38, 0, ["9223372036854775807", "-9223372036854775808", None])
    assert call(a, False, False).to_pylist() == [9223372036854775807, -9223372036854775808, None]
    check_cast(sess, a, *unscaled(a), i64, False, False)
    for beyond in ("9223372036854775808", "-9223372036854775809"):
        with pytest.raises(Exception, match=BOUNDS):
            call(dec_arr(width, 38, 0, [beyond]), False, False)


@pytest.mark.gpu
def test_reference_integer_to_decimal_table(sess):
    """TestIntegerToDecimal (compute/cast_test.go:877-911)"""
    for width in (128, 256):
        to = dec_type(width, 22, 2)
        for it in INT_TYPES:
            a = pa.array([0, 7, None, 100, 99], it)
            got = sess.call_function("cast", [a], "to_type=" + fmt(to))
            assert got.type == to and got.to_pylist() == [D("0.00"), D("7.00"), None, D("100.00"), D("99.00")], (it, to)
            check_cast(sess, a, [0, 7, 0, 100, 99], [1, 1, 0, 1, 1], to)
        a = pa.array([-9223372036854775808, 9223372036854775807], pa.int64())
        assert sess.call_function("cast", [a], "to_type=" + fmt(dec_type(width, 19, 0))).to_pylist() == [D(-9223372036854775808), D(9223372036854775807)]
        a = pa.array([0, 18446744073709551615], pa.uint64())
        assert sess.call_function("cast", [a], "to_type=" + fmt(dec_type(width, 20, 0))).to_pylist() == [D(0), D(18446744073709551615)]
    # insufficient output precision: decided from the types, a column of zeros fails
    with pytest.raises(Exception, match="precision is not great enough for result. It should be at least 6"):
        sess.call_function("cast", [pa.array([0], pa.int8())], "to_type=d:5,3")
    with pytest.raises(Exception, match="precision is not great enough for result. It should be at least 77"):
        sess.call_function("cast", [pa.array([0], pa.int32())], "to_type=d:76,67,256")
    with pytest.raises(Exception, match="precision is not great enough"):
        sess.call_function("cast", [pa.array([], pa.int8())], "to_type=d:5,3")          # … before any row is read


@pytest.mark.gpu
@pytest.mark.parametrize("win,wout", [(128, 128), (256, 256), (128, 256), (256, 128)])
def test_reference_decimal_to_decimal_tables(sess, win, wout):
    """TestDecimal128ToDecimal128 / 256ToDecimal256 / 128ToDecimal256 / 256ToDecimal128 (compute/cast_test.go:913-1255)"""
    def cast(a, to, trunc):
        return sess.call_function("cast", [a], opt_text(to, trunc))
    wide_p = 42 if win == 256 and wout == 128 else 38
    for trunc in (False, True):
        # round trip between scales
        no_trunc = dec_arr(win, wide_p, 10, ["02.0000000000", "30.0000000000", "22.0000000000", "-121.0000000000", None])
        out_s = 0 if (win, wout) == (256, 128) else 10
        expected = dec_arr(wout, 28, out_s, ["02.", "30.", "22.", "-121.", None])
        assert cast(no_trunc, expected.type, trunc).equals(expected)
        assert cast(expected, no_trunc.type, trunc).equals(no_trunc)
        check_cast(sess, no_trunc, *unscaled(no_trunc), expected.type, trunc)
        check_cast(sess, expected, *unscaled(expected), no_trunc.type, trunc)
        # same scale, different precision
        d52 = dec_arr(win, 42 if (win, wout) == (256, 128) else 5, 2, ["12.34", "0.56"])
        d42 = dec_arr(wout, 4, 2, ["12.34", "0.56"])
        assert cast(d52, d42.type, trunc).equals(d42) and cast(d42, d52.type, trunc).equals(d52)
        if wout == 256:
            d402 = dec_arr(256, 40, 2, ["12.34", "0.56"])
            assert cast(d52, d402.type, trunc).equals(d402)
    # rescale leads to trunc
    src = dec_arr(win, 52 if win == 256 and wout == 128 else 38, 10, ["-02.1234567890", "30.1234567890", None])
    p28 = dec_arr(wout, 28, 0, ["-02.", "30.", None])
    round_tripped = dec_arr(256 if 256 in (win, wout) else 128, 38, 10, ["-02.0000000000", "30.0000000000", None])
    assert cast(src, p28.type, True).equals(p28)
    assert cast(p28, round_tripped.type, True).equals(round_tripped)
    with pytest.raises(Exception, match=LOSS):
        cast(src, p28.type, False)
    assert cast(p28, round_tripped.type, False).equals(round_tripped)
    check_cast(sess, src, *unscaled(src), p28.type, True)
    check_cast(sess, src, *unscaled(src), p28.type, False)
    # precision loss without rescale = trunc; 12.34 as decimal(4,2) → decimal(3,2) fails although the scales are equal
    d42 = dec_arr(win, 4, 2, ["12.34"])
    for p, s in ((3, 2), (4, 3), (2, 1)):
        to = dec_type(wout, p, s)
        cast(d42, to, True)
        with pytest.raises(Exception, match=NOFIT if s >= 2 else LOSS):
            cast(d42, to, False)
        check_cast(sess, d42, *unscaled(d42), to, True)
        check_cast(sess, d42, *unscaled(d42), to, False)


# ---- random parity ----------------------------------------------------------------------------------------------------------------------
def random_slots(rng, n, bits, digits):
    """unscaled integers of up to `digits` digits, with edges"""
    out = []
    for _ in range(n):
        d = int(rng.integers(0, digits + 1))
        v = int("".join(str(int(x)) for x in rng.integers(0, 10, d)) or "0") if d else 0
        out.append(-v if rng.random() < 0.5 else v)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("win,wout", [(128, 128), (256, 256), (128, 256), (256, 128)])
def test_random_rescale_parity(sess, win, wout):
    """scale deltas −38 … +38 (to ±76 where a 256-bit side can hold them), 0 / 10 / 100 % nulls, sliced inputs (offset 3 and 64),
    lengths 0, 1, 63, 64, 65, garbage under nulls that would fail if looked at; safe and truncating"""
    rng = np.random.default_rng(win * 1000 + wout)
    pin, pout = (38 if win == 128 else 76), (38 if wout == 128 else 76)
    kmax = 38 if win == 128 and wout == 128 else 76
    lengths = [0, 1, 63, 64, 65, 200]
    case = 0
    for delta in list(range(-kmax, kmax + 1)):
        in_scale = max(0, -delta) if delta < 0 else int(rng.integers(0, max(1, min(pin, pout - delta) // 2 + 1)))
        out_scale = in_scale + delta
        if out_scale > pout or in_scale > pin:
            continue
        n = lengths[case % len(lengths)]
        null_frac = (0.0, 0.1, 1.0)[(case // 2) % 3]
        offset = (0, 3, 64)[case % 3]
        case += 1
        valid = [0 if rng.random() < null_frac else 1 for _ in range(n)]
        for trunc in (False, True):
            # safe: digits chosen so that most columns pass — multiples of 10^−delta on a downscale, products inside the precision
            out_p = pout - 1 if delta == 0 and win == wout else pout     # (an identical type would return the input itself)
            room = out_p - max(delta, 0)
            slots = random_slots(rng, n, win, max(0, min(pin, room if not trunc else pin)))
            if delta < 0 and not trunc:
                slots = [to_signed(v * 10 ** -delta, 1024) for v in random_slots(rng, n, win, max(0, pin + delta))]
            # garbage under nulls: the widest magnitude of the width, which loses data and overflows every precision
            slots = [v if ok else ((1 << (win - 1)) - 1 - int(rng.integers(0, 9))) for v, ok in zip(slots, valid)]
            arr = make_array(dec_type(win, pin, in_scale), slots, valid, offset)
            check_cast(sess, arr, slots, valid, dec_type(wout, out_p, out_scale), trunc)
    # the big column: 2^20 + 3 rows, values inside int64 so that numpy restates it; sliced at an offset that is no multiple of 8
    n = (1 << 20) + 3
    v = rng.integers(-10 ** 15, 10 ** 15, n + 5, dtype=np.int64)
    ok = rng.random(n + 5) >= 0.1
    limbs_in = np.empty((n + 5, win // 64), np.int64)
    limbs_in[:, 0] = v
    limbs_in[:, 1:] = (v >> 63)[:, None]
    limbs_in[~ok] = -7                                     # garbage under nulls
    arr = pa.Array.from_buffers(dec_type(win, 20, 1), n, [pa.py_buffer(np.packbits(ok, bitorder="little").tobytes()), pa.py_buffer(limbs_in.tobytes())],
                                null_count=int((~ok[5:]).sum()), offset=5)
    got = sess.call_function("cast", [arr], "to_type=" + fmt(dec_type(wout, 22, 3)))
    exp = np.empty((n, wout // 64), np.int64)
    exp[:, 0] = v[5:] * 100
    exp[:, 1:] = ((v[5:] * 100) >> 63)[:, None]
    exp[~ok[5:]] = 0
    assert got.buffers()[1].to_pybytes()[:n * wout // 8] == exp.tobytes()
    assert got.null_count == int((~ok[5:]).sum())
    assert np.array_equal(np.unpackbits(np.frombuffer(got.buffers()[0], np.uint8), bitorder="little")[:n].astype(bool), ok[5:])


@pytest.mark.gpu
def test_unsafe_upscale_that_leaves_the_width_wraps_and_safe_refuses(sess):
    """the reference's FromBigInt panics here (decimal128.go:78-82); decision: safe → "does not fit in precision", unsafe → modulo 2^128 /
    2^256, which is what Arrow C++ returns (38 nines × 100 = 1318113592927845595621363844787218676.76)"""
    nines = 10 ** 38 - 1
    a = make_array(pa.decimal128(38, 0), [nines, -nines, 1], [1, 1, 1])
    got = sess.call_function("cast", [a], "to_type=d:38,2;allow_decimal_truncate=1")
    assert got.to_pylist()[0] == D("1318113592927845595621363844787218676.76")
    check_cast(sess, a, [nines, -nines, 1], [1, 1, 1], pa.decimal128(38, 2), True)
    with pytest.raises(Exception, match=NOFIT):
        sess.call_function("cast", [a], "to_type=d:38,2")
    big = 10 ** 76 - 1
    b = make_array(pa.decimal256(76, 0), [big, -big, 5], [1, 1, 1])
    check_cast(sess, b, [big, -big, 5], [1, 1, 1], pa.decimal256(76, 30), True)
    with pytest.raises(Exception, match=NOFIT):
        sess.call_function("cast", [b], "to_type=d:76,30,256")
    # a product that leaves 2^256 altogether (carry out of the top limb) is refused the same way
    c = make_array(pa.decimal256(76, 0), [(1 << 255) - 1], [1])
    with pytest.raises(Exception, match=NOFIT):
        sess.call_function("cast", [c], "to_type=d:76,40,256")


@pytest.mark.gpu
@pytest.mark.parametrize("width", [128, 256])
def test_random_integer_decimal_parity(sess, width):
    """every integer type → decimal → the same integer type, at the types' extremes.  One more place where Arrow C++ parts from the
    reference turned up here: a SAFE Decimal256 → uint64 cast of a value in [2^63, 2^64) at a scale > 0 (18446744073709551615 · 10^19
    at scale 19) is refused by pyarrow with "Rescaling Decimal value would cause data loss" although the division is exact; the
    reference (big.Int QuoRem, decimal256.go Rescale) and the restatement return the value.  Those columns are checked by the
    restatement alone, and the same columns halved (every value below 2^63) are checked against pyarrow as well."""
    rng = np.random.default_rng(width + 1)
    pmax = 38 if width == 128 else 76
    for it in INT_TYPES:
        bits = it.bit_width
        signed = pa.types.is_signed_integer(it)
        lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
        digits = MAX_DIGITS.get(bits, 19 if signed else 20)
        for n, null_frac, offset in ((0, 0, 0), (1, 0, 0), (63, 0.1, 3), (64, 1.0, 0), (65, 0.1, 64), (300, 0.1, 5)):
            vals = [lo, hi, 0, 1, hi - 1][:n] + [int(rng.integers(lo, hi, endpoint=True, dtype=np.int64 if signed else np.uint64)) for _ in range(max(0, n - 5))]
            valid = [0 if rng.random() < null_frac else 1 for _ in range(n)]
            scale = int(rng.integers(0, pmax - digits + 1))
            a = make_array(it, vals, valid, offset)
            check_cast(sess, a, vals, valid, dec_type(width, digits + scale, scale))
            # and back: decimal → this integer type, safe; the values fit, the scale divides exactly
            back = [v * 10 ** scale for v in vals]
            garbage = [v if ok else (1 << (width - 2)) + 3 for v, ok in zip(back, valid)]     # out of bounds AND lossy under nulls
            d = make_array(dec_type(width, pmax, scale), garbage, valid, offset)
            agree = not (width == 256 and it == pa.uint64())
            check_cast(sess, d, garbage, valid, it, False, False, against_pyarrow=agree)
            check_cast(sess, d, garbage, valid, it, True, True, against_pyarrow=agree)
            if not agree:
                halved = [(v >> 1) * 10 ** scale if ok else g for v, ok, g in zip(vals, valid, garbage)]
                d = make_array(dec_type(width, pmax, scale), halved, valid, offset)
                check_cast(sess, d, halved, valid, it, False, False)
                check_cast(sess, d, halved, valid, it, True, True)
    # out of range for a narrow target, wrapped with allow_int_overflow
    d = make_array(dec_type(width, 20, 1), [3000, -1290, 2550, 70], [1, 1, 1, 1])
    for it in INT_TYPES:
        check_cast(sess, d, [3000, -1290, 2550, 70], [1, 1, 1, 1], it, False, False)
        check_cast(sess, d, [3000, -1290, 2550, 70], [1, 1, 1, 1], it, False, True)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [128, 256])
def test_decimal_to_int_truncate_rounds_half_away_from_zero(sess, width):
    """the rows pyarrow is NOT asked about: Arrow C++ truncates (2.50 → 2), the reference's ReduceScaleBy(scale, true) rounds half
    away from zero (2.50 → 3, −2.50 → −3) — DESIGN.md "Reference quirks — decisions".  Restatement alone."""
    rows = [250, -250, 249, -249, 251, -251, 50, -50, 49, -49, 99, -99, 150, -150, 0]
    a = make_array(dec_type(width, 10, 2), rows, [1] * len(rows))
    got = sess.call_function("cast", [a], "to_type=int64;allow_decimal_truncate=1")
    assert got.to_pylist() == [3, -3, 2, -2, 3, -3, 1, -1, 0, 0, 1, -1, 2, -2, 0]
    assert pc.cast(a, options=pc.CastOptions(pa.int64(), allow_decimal_truncate=True)).to_pylist()[:2] == [2, -2]     # the other opinion
    check_cast(sess, a, rows, [1] * len(rows), pa.int64(), True, False, against_pyarrow=False)
    rng = np.random.default_rng(width)
    pmax = 38 if width == 128 else 76
    for scale in (1, 5, 19, 20, pmax):
        vals = [int(rng.integers(-10 ** 9, 10 ** 9)) * 10 ** scale + s * int(rng.integers(5, 10)) * 10 ** (scale - 1) + s * int(rng.integers(0, 10 ** min(scale - 1, 18)))
                for s in (1, -1) for _ in range(100)]
        vals = [v for v in vals if abs(v) < 10 ** pmax]
        a = make_array(dec_type(width, pmax, scale), vals, [1] * len(vals))
        check_cast(sess, a, vals, [1] * len(vals), pa.int64(), True, False, against_pyarrow=False)


@pytest.mark.gpu
def test_error_order_is_row_order(sess):
    """a data-loss row before and after a precision-overflow row reports the first; with that row nulled, the next"""
    t = pa.decimal128(10, 3)
    slots = [1000, 2005, 99999999000, 3007, 4000]          # row 1 loses data (→ scale 2), row 2 exceeds decimal(6,2), row 3 loses data
    to = "to_type=d:6,2"
    with pytest.raises(Exception, match=LOSS):
        sess.call_function("cast", [make_array(t, slots, [1, 1, 1, 1, 1])], to)
    with pytest.raises(Exception, match=NOFIT):
        sess.call_function("cast", [make_array(t, slots, [1, 0, 1, 1, 1])], to)
    with pytest.raises(Exception, match=LOSS):
        sess.call_function("cast", [make_array(t, slots, [1, 0, 0, 1, 1])], to)
    ok = sess.call_function("cast", [make_array(t, slots, [1, 0, 0, 0, 1])], to)
    assert slots_of(ok) == ([100, 0, 0, 0, 400], [True, False, False, False, True], 3)
    # far apart, so that different workgroups find them
    n = 1 << 18
    big = [1000] * n
    big[70000], big[9000], big[200000] = 2005, 99999999000, 2005
    with pytest.raises(Exception, match=NOFIT):
        sess.call_function("cast", [make_array(t, big, [1] * n)], to)
    big[100] = 3007
    with pytest.raises(Exception, match=LOSS):
        sess.call_function("cast", [make_array(t, big, [1] * n)], to)


@pytest.mark.gpu
def test_identity_scalars_refusals_and_chunked(sess):
    a = pa.array([D("1.5"), None, D("-2.5")], pa.decimal128(5, 1))
    # an identical type returns its input; a different scale of the same type id reaches a kernel
    assert sess.call_function("cast", [a], "to_type=d:5,1").equals(a)
    assert sess.call_function("cast", [a], "to_type=d:5,2").to_pylist() == [D("1.50"), None, D("-2.50")]
    assert sess.call_function("cast", [a], "to_type=d:5,2").type == pa.decimal128(5, 2)
    # negative scales on decimal → decimal: refused
    with pytest.raises(Exception, match="negative scales not supported"):
        sess.call_function("cast", [make_array(pa.decimal128(5, -1), [1], [1])], "to_type=d:5,1")
    # out of scope: float / string / bool ↔ decimal
    for bad in (pa.array([1.5], pa.float64()), pa.array(["1"], pa.string()), pa.array([True], pa.bool_())):
        with pytest.raises(Exception, match="unsupported cast"):
            sess.call_function("cast", [bad], "to_type=d:5,1")
    with pytest.raises(Exception, match="unsupported cast"):
        sess.call_function("cast", [a], "to_type=double")
    # safe=0 sets allow_decimal_truncate
    assert sess.call_function("cast", [a], "to_type=d:5,0;safe=0").to_pylist() == [D("1"), None, D("-2")]
    # a chunked column of three uneven chunks equals the concatenated cast
    rng = np.random.default_rng(3)
    vals = [None if rng.random() < 0.1 else D(int(rng.integers(-10 ** 9, 10 ** 9))).scaleb(-2) for _ in range(1000)]
    whole = pa.array(vals, pa.decimal128(20, 2))
    ca = pa.chunked_array([whole[:1], whole[1:130], whole[130:]])
    for to in ("d:30,5", "d:30,5,256", "int64;allow_decimal_truncate=1"):
        got = sess.call_function("cast", [ca], "to_type=" + to)
        one = sess.call_function("cast", [whole], "to_type=" + to)
        assert isinstance(got, pa.ChunkedArray) and [len(c) for c in got.chunks] == [1, 129, 870]
        assert got.combine_chunks().equals(one) if got.num_chunks else True
    ints = pa.chunked_array([pa.array([1, None], pa.int32()), pa.array([3], pa.int32()), pa.array([4, 5, 6, 7], pa.int32())])
    assert sess.call_function("cast", [ints], "to_type=d:12,2").combine_chunks().to_pylist() == [D("1.00"), None, D("3.00"), D("4.00"), D("5.00"), D("6.00"), D("7.00")]


# ---- the C ABI, and size ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("win,wout", [(16, 16), (32, 32), (16, 32), (32, 16)])
def test_sixteen_million_rows_byte_equal_through_the_c_abi(ctx, win, wout):
    """2^24 rows per width pair through ah_cast_decimal_rescale, safe, × 10^2, 10 % nulls over garbage; numpy restates it (the values
    lie inside int64).  Then the same column ÷ 10^2 back, and integer → decimal → integer through the other two entry points."""
    n = 1 << 24
    rng = np.random.default_rng(win + wout)
    v = rng.integers(-10 ** 15, 10 ** 15, n, dtype=np.int64)
    ok = rng.random(n) >= 0.1
    vbits = np.packbits(ok, bitorder="little")

    def limbs(x, w, nulls_as):
        a = np.empty((n, w // 8), np.int64)
        a[:, 0] = x
        a[:, 1:] = (x >> 63)[:, None]
        a[~ok] = nulls_as
        return a

    d_in = ctx.to_device(limbs(v, win, -3).view(np.uint8).reshape(-1))
    d_valid = ctx.to_device(vbits)
    d_out = ctx.alloc(n * wout)
    ctx.cast_decimal_rescale(win, wout, 2, 20, False, d_in, d_valid, 0, n, d_out)
    assert d_out.download(np.uint8, n * wout).tobytes() == limbs(v * 100, wout, 0).tobytes()
    # back down: exact, so the safe cast passes; the garbage under nulls (−3) would lose data if it were read
    d_back = ctx.alloc(n * win)
    ctx.cast_decimal_rescale(wout, win, -2, 20, False, d_out, d_valid, 0, n, d_back)
    assert d_back.download(np.uint8, n * win).tobytes() == limbs(v, win, 0).tobytes()
    # integer → decimal (× 10^3) → integer (÷ 10^3, safe, range-checked)
    d_int = ctx.to_device(np.where(ok, v, 77))
    ctx.cast_int_to_decimal(9, wout, 3, d_int, d_valid, 0, n, d_out)
    assert d_out.download(np.uint8, n * wout).tobytes() == limbs(v * 1000, wout, 0).tobytes()
    d_i2 = ctx.alloc(n * 8)
    ctx.cast_decimal_to_int(wout, 3, 9, False, False, d_out, d_valid, 0, n, d_i2)
    assert np.array_equal(d_i2.download(np.int64, n), np.where(ok, v, 0))
