"""String casts through `cast`: String / Binary / LargeString / LargeBinary → the eight integer types and Boolean (strconv.ParseInt /
ParseUint / ParseBool), integers and Boolean → String / LargeString (strconv.FormatInt / FormatUint / FormatBool), the binary-like ↔
binary-like casts with UTF-8 validation, and FixedSizeBinary → binary-like (kernels/numeric_cast.go:742-781, boolean_cast.go:77-95,
string_casts.go; cast_string … cast_fixed_sized_binary: compute/cast.go:906-912).

Expected values never come from the code under test: Python itself (str(v), bytes.decode), tests/strconv_model.py (Go's rules restated,
pinned by the reference's vectors in tests/test_strconv_host.py), the reference's tables (compute/cast_test.go), transcribed, and
pyarrow.compute.cast as a third opinion where Arrow C++ and the reference agree.  Every column comes without nulls and with ≈ 10 % of
them, sliced at array offset 3, with 4- and 8-byte offsets.

Not tested, covered by reading: a formatted total above INT32_MAX and the reference's reservation bound — both need
columns of several GiB."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from tests import strconv_model as M

INT_TYPES = [pa.int8(), pa.uint8(), pa.int16(), pa.uint16(), pa.int32(), pa.uint32(), pa.int64(), pa.uint64()]
TYPE_IDS = {"uint8": 2, "int8": 3, "uint16": 4, "int16": 5, "uint32": 6, "int32": 7, "uint64": 8, "int64": 9}
STRINGS = [pa.string(), pa.large_string()]
BINARY_LIKE = [pa.string(), pa.binary(), pa.large_string(), pa.large_binary()]
ROWS = [0, 1, 63, 64, 65, 1000, 70001]
OFF = 3
FMT = {pa.string(): "string", pa.large_string(): "large_string", pa.binary(): "binary", pa.large_binary(): "large_binary", pa.bool_(): "bool"}


def fmt(t):
    if pa.types.is_fixed_size_binary(t):
        return "w:%d" % t.byte_width
    return FMT.get(t, str(t))


def offset_width(t):
    return 8 if t in (pa.large_string(), pa.large_binary()) else 4


def validity_buffer(valid, offset):
    bits = np.ones(offset + len(valid), np.uint8)
    bits[offset:] = np.asarray(valid, np.uint8)
    return pa.py_buffer(np.packbits(bits, bitorder="little").tobytes())


def bytes_array(typ, rows, valid=None, offset=OFF):
    """a binary-like or fixed-size binary column of `rows` (bytes) at array offset `offset`, its payload kept under the null slots"""
    junk = b"\xfe\xff\xfe" if pa.types.is_fixed_size_binary(typ) else b"\xffjunk\xfe"
    full = [junk] * offset + list(rows)
    carrier = typ if pa.types.is_fixed_size_binary(typ) else (pa.large_binary() if offset_width(typ) == 8 else pa.binary())
    base = pa.array(full, carrier)
    nulls = 0 if valid is None else int(len(valid) - sum(valid))
    vbuf = None if valid is None else validity_buffer(valid, offset)
    return pa.Array.from_buffers(typ, len(rows), [vbuf] + base.buffers()[1:], null_count=nulls, offset=offset)


def int_array(typ, values, valid=None, offset=OFF):
    npdt = np.dtype(typ.to_pandas_dtype())
    data = np.concatenate([np.full(offset, 0x5A, npdt), np.array([v & ((1 << typ.bit_width) - 1) for v in values], np.uint64).astype(npdt)])
    nulls = 0 if valid is None else int(len(valid) - sum(valid))
    vbuf = None if valid is None else validity_buffer(valid, offset)
    return pa.Array.from_buffers(typ, len(values), [vbuf, pa.py_buffer(data.tobytes())], null_count=nulls, offset=offset)


def bool_array(values, valid=None, offset=OFF):
    bits = np.concatenate([np.array([1, 0, 1][:offset], np.uint8), np.asarray(values, np.uint8)])
    nulls = 0 if valid is None else int(len(valid) - sum(valid))
    vbuf = None if valid is None else validity_buffer(valid, offset)
    return pa.Array.from_buffers(pa.bool_(), len(values), [vbuf, pa.py_buffer(np.packbits(bits, bitorder="little").tobytes())], null_count=nulls, offset=offset)


def mask(n, with_nulls, seed):
    if not with_nulls:
        return None
    return (np.random.default_rng(seed).random(n) >= 0.1).astype(np.uint8).tolist()


def rows_of(arr):
    """(bytes of every row, offsets of the rows as stored, validity list) of a binary-like result — null rows read like the others"""
    n = len(arr)
    bufs = arr.buffers()
    ow = offset_width(arr.type)
    offs = np.frombuffer(bufs[1], np.int64 if ow == 8 else np.int32)[arr.offset:arr.offset + n + 1]
    data = bufs[2].to_pybytes() if bufs[2] is not None else b""
    rows = [data[offs[i]:offs[i + 1]] for i in range(n)]
    if bufs[0] is None:
        valid = [True] * n
    else:
        valid = [bool(b) for b in np.unpackbits(np.frombuffer(bufs[0], np.uint8), bitorder="little")[arr.offset:arr.offset + n]]
    return rows, offs, valid


def slots_of(arr):
    """(value of every slot, validity list) of an integer result"""
    n = len(arr)
    bufs = arr.buffers()
    vals = np.frombuffer(bufs[1], np.dtype(arr.type.to_pandas_dtype()))[arr.offset:arr.offset + n].tolist()
    if bufs[0] is None:
        return vals, [True] * n
    return vals, [bool(b) for b in np.unpackbits(np.frombuffer(bufs[0], np.uint8), bitorder="little")[arr.offset:arr.offset + n]]


def bits_of(arr):
    n = len(arr)
    bufs = arr.buffers()
    data = np.unpackbits(np.frombuffer(bufs[1], np.uint8), bitorder="little")[arr.offset:arr.offset + n].tolist()
    if bufs[0] is None:
        return data, [True] * n
    return data, [bool(b) for b in np.unpackbits(np.frombuffer(bufs[0], np.uint8), bitorder="little")[arr.offset:arr.offset + n]]


@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.close()


def cast(sess, arr, to, extra=""):
    got = sess.call_function("cast", [arr], "to_type=" + fmt(to) + extra)
    assert got.type == to, (got.type, to)
    return got


# ---- the reference's vectors ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("stype", BINARY_LIKE)
def test_reference_string_to_int(sess, stype):
    """TestStringToInt (compute/cast_test.go:2542-2579); the Binary inputs run the same kernels (numeric_cast.go:815-833)"""
    for t in INT_TYPES:
        acc = [(s, v) for tt, s, v in M.GOLDEN_ACCEPTED if tt == str(t)]
        rows = [s for s, _ in acc]
        rows.insert(1, b"not a number")       # … under the null the reference's tables have in second place
        valid = [1] * len(rows)
        valid[1] = 0
        got = cast(sess, bytes_array(stype, rows, valid), t)
        want = [v for _, v in acc]
        want.insert(1, None)
        assert got.to_pylist() == want, (stype, t)
        assert slots_of(got)[0][1] == 0
    for s, kind in zip(M.GOLDEN_NOT_INT8, [M.SYNTAX, M.SYNTAX, M.RANGE, M.RANGE, M.SYNTAX, M.SYNTAX, M.RANGE, M.RANGE]):
        with pytest.raises(Exception) as e:
            cast(sess, bytes_array(stype, [s]), pa.int8())
        assert M.parse_error_text("int8", s, kind) in str(e.value), (s, str(e.value))
    for s, kind in zip(M.GOLDEN_NOT_UINT8, [M.RANGE, M.SYNTAX, M.SYNTAX, M.SYNTAX, M.SYNTAX, M.RANGE]):
        with pytest.raises(Exception) as e:
            cast(sess, bytes_array(stype, [s]), pa.uint8())
        assert M.parse_error_text("uint8", s, kind) in str(e.value), (s, str(e.value))


@pytest.mark.gpu
@pytest.mark.parametrize("stype", STRINGS)
def test_reference_int_and_bool_to_string(sess, stype):
    """TestIntToString, TestBooleanToString (compute/cast_test.go:3202-3268)"""
    for t in INT_TYPES:
        bits = t.bit_width
        vals = [0, 1, (1 << (bits - 1)) - 1, -(1 << (bits - 1)), None] if pa.types.is_signed_integer(t) else [0, 1, (1 << bits) - 1, None]
        got = cast(sess, pa.array(vals, t), stype)
        assert got.to_pylist() == [None if v is None else str(v) for v in vals], (t, stype)
    got = cast(sess, pa.array([True, True, False, None], pa.bool_()), stype)
    assert got.to_pylist() == ["true", "true", "false", None]
    assert cast(sess, pa.array([], pa.int32()), stype).to_pylist() == []


@pytest.mark.gpu
def test_parse_bool_spellings(sess):
    rows = M.TRUE_SPELLINGS + M.FALSE_SPELLINGS
    for stype in BINARY_LIKE:
        got = cast(sess, bytes_array(stype, rows), pa.bool_())
        assert got.to_pylist() == [True] * 6 + [False] * 6
    for bad in (b"", b"TRUE ", b"tRUE", b"yes", b"2"):
        with pytest.raises(Exception) as e:
            cast(sess, bytes_array(pa.string(), rows + [bad]), pa.bool_())
        assert M.parse_error_text("bool", bad, M.SYNTAX) in str(e.value), (bad, str(e.value))


# ---- round trips and parity -----------------------------------------------------------------------------------------------------
def random_values(t, n, rng):
    bits = t.bit_width
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if pa.types.is_signed_integer(t) else (0, (1 << bits) - 1)
    vals = [lo, hi, 0, 1, lo + 1, hi - 1, 9, 10, 99, 100][:n]
    while len(vals) < n:
        # every number of digits equally often, so every length of the output occurs
        mag = int(rng.integers(0, 1 << int(rng.integers(1, bits + 1)), dtype=np.uint64)) if bits == 64 else int(rng.integers(0, 1 << int(rng.integers(1, bits + 1))))
        v = -mag if (lo < 0 and rng.random() < 0.5) else mag
        vals.append(min(max(v, lo), hi))
    return vals


@pytest.mark.gpu
@pytest.mark.parametrize("with_nulls", [False, True])
@pytest.mark.parametrize("n", ROWS)
def test_integer_string_round_trip(sess, n, with_nulls):
    rng = np.random.default_rng(n * 2 + with_nulls)
    valid = mask(n, with_nulls, n)
    for k, t in enumerate(INT_TYPES):
        vals = random_values(t, n, rng)
        arr = int_array(t, vals, valid)
        texts = [str(v).encode() if (valid is None or valid[i]) else b"" for i, v in enumerate(vals)]
        for stype in (STRINGS if n <= 1000 else [STRINGS[k % 2]]):
            got = cast(sess, arr, stype)
            rows, offs, gvalid = rows_of(got)
            assert rows == texts, (t, stype, n)
            assert offs.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in texts])]).astype(np.int64).tolist()
            assert gvalid == ([True] * n if valid is None else list(map(bool, valid)))
            ref = pa.array([v if (valid is None or valid[i]) else None for i, v in enumerate(vals)], t)
            assert got.to_pylist() == pc.cast(ref, stype).to_pylist(), (t, stype, n)
            # … and back: the string column the device made, sliced again so that its offsets start mid-buffer
            back = cast(sess, got, t)
            bvals, bvalid = slots_of(back)
            assert bvals == [v if (valid is None or valid[i]) else 0 for i, v in enumerate(vals)], (t, stype, n)
            assert bvalid == gvalid
            if n > OFF:
                assert cast(sess, got.slice(OFF), t).to_pylist() == ref.slice(OFF).to_pylist()


@pytest.mark.gpu
@pytest.mark.parametrize("with_nulls", [False, True])
@pytest.mark.parametrize("n", ROWS)
def test_boolean_string_round_trip(sess, n, with_nulls):
    rng = np.random.default_rng(7 * n + with_nulls)
    vals = rng.integers(0, 2, n).tolist()
    valid = mask(n, with_nulls, n + 1)
    arr = bool_array(vals, valid)
    texts = [(b"true" if v else b"false") if (valid is None or valid[i]) else b"" for i, v in enumerate(vals)]
    for stype in STRINGS:
        got = cast(sess, arr, stype)
        rows, offs, gvalid = rows_of(got)
        assert rows == texts and offs[0] == 0 and gvalid == ([True] * n if valid is None else list(map(bool, valid)))
        assert got.to_pylist() == pc.cast(arr, stype).to_pylist()
        back = cast(sess, got, pa.bool_())
        data, bvalid = bits_of(back)
        assert data == [int(v) if (valid is None or valid[i]) else 0 for i, v in enumerate(vals)] and bvalid == gvalid


@pytest.mark.gpu
@pytest.mark.parametrize("t", INT_TYPES, ids=str)
def test_parse_matches_the_restatement_on_arbitrary_strings(sess, t):
    """every row that Go accepts, in one column: prefixes, underscores, signs, leading zeros, rows far longer than a number"""
    import random
    rng = random.Random(TYPE_IDS[str(t)])
    alphabet = b"0123456789abcdefxXbo_+-z"
    cand = [bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 12))) for _ in range(6000)]
    cand += [b"0" * 299 + b"7", b"0x" + b"0" * 70 + b"1f", b"0b" + b"0_" * 40 + b"1", b"-0", b"+0", b"00", b"0_7", b"0x_1", b"1_000"]
    bits = t.bit_width
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if pa.types.is_signed_integer(t) else (0, (1 << bits) - 1)
    for v in (lo, hi, lo - 1, hi + 1):        # the two ends and the first value past each, the latter out of range in every base
        cand += [("%s0x%x" % ("-" if v < 0 else "", abs(v))).encode(), ("%s0B%s" % ("-" if v < 0 else "", bin(abs(v))[2:])).encode(),
                 ("%s0%o" % ("-" if v < 0 else "", abs(v))).encode(), ("%s0o%o" % ("-" if v < 0 else "", abs(v))).encode(), str(v).encode()]
    # random text is seldom a number of a narrow type, so the column is filled up from Go's grammar itself: a value of every number of
    # bits, in every base and prefix case, with an explicit sign, leading zeros and underscores between the digits
    for _ in range(400):
        mag = rng.randrange(1 << rng.randint(1, bits))
        v = -mag if (lo < 0 and rng.random() < 0.5) else mag
        v = min(max(v, lo), hi)
        prefix, digits = rng.choice([("", "%d"), ("0x", "%x"), ("0X", "%X"), ("0b", "{:b}"), ("0B", "{:b}"), ("0o", "%o"), ("0O", "%o"), ("0", "%o")])
        text = digits.format(abs(v)) if "{" in digits else digits % abs(v)
        if prefix and rng.random() < 0.3:
            text = "0" * rng.randint(1, 4) + text
        if len(text) > 1 and rng.random() < 0.3:
            k = rng.randrange(1, len(text))
            text = text[:k] + "_" + text[k:]
        if prefix and rng.random() < 0.2:
            text = "_" + text                                   # directly after the base prefix
        sign = "-" if v < 0 else ("+" if (lo < 0 and rng.random() < 0.2) else "")
        made = (sign + prefix + text).encode()
        assert M.go_parse(str(t), made)[:2] == (v, None), made
        cand.append(made)
    parsed = [(s, M.go_parse(str(t), s)) for s in cand]
    good = [(s, r[0]) for s, r in parsed if r[1] is None]
    assert len(good) > 300
    for stype in (pa.string(), pa.large_binary()):
        got = cast(sess, bytes_array(stype, [s for s, _ in good]), t)
        assert got.to_pylist() == [v for _, v in good]
    # each kind of failure, alone in a column of good rows, quoted as Go quotes it
    bad = [(s, r[1]) for s, r in parsed if r[1] is not None]
    for kind in (M.SYNTAX, M.RANGE):
        s = next(s for s, k in bad if k == kind and s)
        with pytest.raises(Exception) as e:
            cast(sess, bytes_array(pa.string(), [b"1", s, b"2"]), t)
        assert M.parse_error_text(str(t), s, kind) in str(e.value), (s, str(e.value))
    with pytest.raises(Exception) as e:
        cast(sess, bytes_array(pa.string(), [b"1" * 25 + b"z"]), t)      # the overflow comes first in scan order
    assert M.parse_error_text(str(t), b"1" * 25 + b"z", M.RANGE) in str(e.value)


# ---- which row the error names --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 70001])
def test_parse_error_is_the_last_offending_valid_row(sess, n):
    p, q, hidden = n // 5, n // 2 + 7, n - 2
    rows = [str(i % 100).encode() for i in range(n)]
    rows[p], rows[q], rows[hidden] = b"12 z", b"300", b"zzz"
    valid = [1] * n
    valid[hidden] = 0
    for stype in (pa.string(), pa.large_string()):
        with pytest.raises(Exception) as e:
            cast(sess, bytes_array(stype, rows, valid), pa.uint8() if n == 65 else pa.int8())
        assert 'parsing "300": value out of range' in str(e.value), str(e.value)
        ok = list(rows)
        ok[p] = ok[q] = b"5"
        got = cast(sess, bytes_array(stype, ok, valid), pa.int32())     # the offender under the null alone: no error
        assert got.to_pylist() == [None if i == hidden else int(ok[i]) for i in range(n)]
    brows = [b"true"] * n
    brows[p], brows[q], brows[hidden] = b"yes", b"nope", b"never"
    with pytest.raises(Exception) as e:
        cast(sess, bytes_array(pa.binary(), brows, valid), pa.bool_())
    assert 'strconv.ParseBool: parsing "nope": invalid syntax' in str(e.value), str(e.value)
    brows[p] = brows[q] = b"F"
    got = cast(sess, bytes_array(pa.binary(), brows, valid), pa.bool_())
    assert got.to_pylist() == [None if i == hidden else (i not in (p, q)) for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 70001])
def test_utf8_error_is_the_first_offending_valid_row(sess, n):
    p, q, hidden = n // 5, n // 2 + 7, 1
    rows = [("r%dé" % i).encode() for i in range(n)]
    rows[p], rows[q], rows[hidden] = b"ab\xc3", b"\xffq", b"\x80"
    valid = [1] * n
    valid[hidden] = 0
    for btype in (pa.binary(), pa.large_binary()):
        with pytest.raises(Exception) as e:
            cast(sess, bytes_array(btype, rows, valid), pa.string())
        assert "invalid UTF8 bytes: 6162c3" in str(e.value), str(e.value)
        ok = list(rows)
        ok[p] = ok[q] = b"fine"
        got = cast(sess, bytes_array(btype, ok, valid), pa.large_string())
        assert rows_of(got)[0] == ok and got.null_count == 1


# ---- UTF-8 ----------------------------------------------------------------------------------------------------------------------
def py_valid(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


@pytest.mark.gpu
def test_reference_binary_to_string(sess):
    """TestBinaryToString (compute/cast_test.go:1410-1481)"""
    rows = [b"Hi", "olá mundo".encode(), "你好世界".encode(), b"", b"\xa0\xa1"]
    for btype in (pa.binary(), pa.large_binary()):
        for stype in STRINGS:
            assert cast(sess, pa.array([], btype), stype).to_pylist() == []
            masked = cast(sess, bytes_array(btype, rows, [1, 1, 1, 1, 0]), stype)
            assert rows_of(masked)[0][:4] == rows[:4] and masked.null_count == 1 and masked.to_pylist()[:4] == ["Hi", "olá mundo", "你好世界", ""]
            with pytest.raises(Exception, match="invalid UTF8 bytes: a0a1"):
                cast(sess, bytes_array(btype, rows), stype)
            allowed = cast(sess, bytes_array(btype, rows), stype, ";allow_invalid_utf8=1")
            assert rows_of(allowed)[0] == rows
            assert rows_of(cast(sess, bytes_array(btype, rows), stype, ";safe=0"))[0] == rows
    fsb = pa.binary(3)
    frows = [b"Hi!", b"l\xc3\xa1", "你".encode(), b"   ", b"\xa0\xa1\xa2"]
    for stype in STRINGS:
        assert cast(sess, pa.array([], fsb), stype).to_pylist() == []
        masked = cast(sess, bytes_array(fsb, frows, [1, 1, 1, 1, 0]), stype)
        assert masked.to_pylist() == ["Hi!", "lá", "你", "   ", None]
        with pytest.raises(Exception, match="invalid UTF8 bytes: a0a1a2"):
            cast(sess, bytes_array(fsb, frows), stype)
        assert rows_of(cast(sess, bytes_array(fsb, frows), stype, ";allow_invalid_utf8=1"))[0] == frows


@pytest.mark.gpu
@pytest.mark.parametrize("btype", [pa.binary(), pa.large_binary()], ids=str)
def test_utf8_validation_by_row_length_and_corruption(sess, btype):
    """valid multi-byte text of 0 … 300 bytes, one byte corrupted at the first, a middle and the last position — each candidate in a
    column of its own between valid neighbours, judged by Python's strict decoder"""
    unit = "aé世\U0001F600bc"     # 1 + 2 + 3 + 4 + 1 + 1 = 12 bytes: sequences straddle every 8-byte boundary sooner or later
    cands = []
    for size in (0, 1, 7, 8, 9, 63, 64, 65, 300):
        text = (unit * 30).encode()
        cut = size
        while cut > 0 and not py_valid(text[:cut]):
            cut -= 1
        row = text[:cut] + b"x" * (size - cut)
        assert len(row) == size and py_valid(row)
        cands.append(row)
        for at in ([0, size // 2, size - 1] if size else []):
            for byte in (0xFF, 0x80, 0xC3, 0xE4):
                cands.append(row[:at] + bytes([byte]) + row[at + 1:])
    cands.append(b"1234567\xe4\xb8\x96")                      # a 3-byte sequence across the first word boundary
    cands.append(b"1234567\xe4\xb8")                          # … cut short
    cands.append(b"123456\xf0\x9f\x98\x80" + b"y" * 70)       # a 4-byte sequence across it, in a row the whole wave shares
    cands.append(b"y" * 15 + b"\xf0\x9f\x98" + b"y" * 70)     # … cut short at a lane's piece boundary
    want = [py_valid(c) for c in cands]
    assert 10 < sum(want) < len(cands) - 10
    good = [c for c, w in zip(cands, want) if w]
    got = cast(sess, bytes_array(btype, good), pa.string())
    assert rows_of(got)[0] == good and got.to_pylist() == [g.decode() for g in good]
    ref = bytes_array(btype, good, offset=0)
    assert got.to_pylist() == pc.cast(ref, pa.string()).to_pylist()
    for c, w in zip(cands, want):
        if w:
            continue
        with pytest.raises(Exception) as e:
            cast(sess, bytes_array(btype, [b"ok", c, "é".encode()]), pa.large_string())
        assert "invalid UTF8 bytes: " + c.hex() in str(e.value), (c, str(e.value))


@pytest.mark.gpu
def test_utf8_rows_are_validated_independently(sess):
    """a row that ends in a cut-short 3-byte sequence and a neighbour that begins with its continuation bytes: read end to end the
    data buffer is valid text"""
    word = "世".encode()
    for btype in (pa.binary(), pa.large_binary()):
        assert py_valid(b"ab" + word[:1] + word[1:] + b"cd")
        with pytest.raises(Exception, match="invalid UTF8 bytes: 6162e4"):
            cast(sess, bytes_array(btype, [b"ab" + word[:1], word[1:] + b"cd"]), pa.string())
        with pytest.raises(Exception, match="invalid UTF8 bytes: b896"):
            cast(sess, bytes_array(btype, [b"ab" + word[:1], word[1:] + b"cd"], [0, 1]), pa.string())
        with pytest.raises(Exception, match="invalid UTF8 bytes: 6162e4"):
            cast(sess, bytes_array(btype, [b"ab" + word[:1], word[1:] + b"cd"], [1, 0]), pa.string())
    with pytest.raises(Exception, match="invalid UTF8 bytes: 6162e4"):
        cast(sess, bytes_array(pa.binary(3), [b"ab" + word[:1], word[1:] + b"c"]), pa.string())


# ---- binary-like ↔ binary-like ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 65, 1000])
def test_binary_like_pairs_match_pyarrow(sess, n):
    rng = np.random.default_rng(n)
    rows = [("v%dé" % int(rng.integers(0, 10 ** int(rng.integers(1, 9))))).encode() * int(rng.integers(0, 3)) for _ in range(n)]
    valid = mask(n, True, n + 5)
    for frm in BINARY_LIKE:
        arr = bytes_array(frm, rows, valid)
        for to in BINARY_LIKE:
            got = sess.call_function("cast", [arr], "to_type=" + fmt(to))
            assert got.type == to
            assert got.to_pylist() == pc.cast(arr, to).to_pylist(), (frm, to, n)
            assert rows_of(got)[0] == rows                      # the payload under the nulls travels with the shared data buffer
    frows = [bytes(rng.integers(0x20, 0x7F, 3, dtype=np.uint8)) for _ in range(n)]
    farr = bytes_array(pa.binary(3), frows, valid)
    for to in BINARY_LIKE:
        got = cast(sess, farr, to)
        assert got.to_pylist() == pc.cast(farr, to).to_pylist(), (to, n)
        assert rows_of(got)[0] == frows
        assert rows_of(got)[1].tolist() == [(OFF + i) * 3 for i in range(n + 1)]     # CastFsbToBinary: (offset + i) · width


@pytest.mark.gpu
def test_string_to_string_and_binary_never_validate(sess):
    """TestStringToString, TestBinaryOrStringToBinary: a string column is taken at its word"""
    rows = [b"Hi", b"\xa0\xa1", b""]
    for frm in STRINGS:
        for to in BINARY_LIKE:
            assert rows_of(sess.call_function("cast", [bytes_array(frm, rows)], "to_type=" + fmt(to)))[0] == rows, (frm, to)
    for frm in (pa.binary(), pa.large_binary()):
        for to in (pa.binary(), pa.large_binary()):
            assert rows_of(sess.call_function("cast", [bytes_array(frm, rows)], "to_type=" + fmt(to)))[0] == rows, (frm, to)


@pytest.mark.gpu
def test_fixed_size_binary_to_fixed_size_binary(sess):
    arr = bytes_array(pa.binary(3), [b"abc", b"def", b"ghi"], [1, 0, 1])
    with pytest.raises(Exception, match=r"failed casting from fixed_size_binary\[3\] to fixed_size_binary\[5\]: widths must match"):
        sess.call_function("cast", [arr], "to_type=w:5")
    same = sess.call_function("cast", [arr], "to_type=w:3")
    assert same.type == pa.binary(3) and same.to_pylist() == [b"abc", None, b"ghi"] and same.offset == OFF


@pytest.mark.gpu
def test_out_of_scope_casts_stay_refused(sess):
    import decimal
    cases = [(pa.array([1.5], pa.float64()), "string"), (pa.array(["1.5"], pa.string()), "double"), (pa.array(["1.5"], pa.string()), "d:5,1"),
             (pa.array([decimal.Decimal("1.5")], pa.decimal128(5, 1)), "string"), (pa.array([1], pa.timestamp("s")), "string"),
             (pa.array([1], pa.int32()), "binary"), (pa.array([1.5], pa.float32()), "large_string")]
    for arr, to in cases:
        with pytest.raises(Exception, match="unsupported cast"):
            sess.call_function("cast", [arr], "to_type=" + to)


@pytest.mark.gpu
def test_chunked_columns_cast_like_their_concatenation(sess):
    vals = list(range(-500, 700, 7))
    vals[3] = vals[90] = None
    whole = pa.array(vals, pa.int64())
    ca = pa.chunked_array([whole.slice(0, 5), whole.slice(5, 100), whole.slice(105)])
    got = sess.call_function("cast", [ca], "to_type=string")
    one = sess.call_function("cast", [whole], "to_type=string")
    assert got.num_chunks == 3 and [len(c) for c in got.chunks] == [5, 100, len(vals) - 105]
    assert got.combine_chunks().to_pylist() == one.to_pylist() == [None if v is None else str(v) for v in vals]
    back = sess.call_function("cast", [got], "to_type=int64")
    assert back.combine_chunks().to_pylist() == vals
    bins = pa.chunked_array([pa.array([b"a", None], pa.binary()), pa.array(["é".encode()], pa.binary()), pa.array([b"xyz", b""], pa.binary())])
    assert sess.call_function("cast", [bins], "to_type=large_string").combine_chunks().to_pylist() == ["a", None, "é", "xyz", ""]


# ---- the kernels at the C ABI ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ow", [4, 8])
def test_entry_points_directly(ctx, ow):
    from arrow_go_amd import _native as N
    n = 1000
    rng = np.random.default_rng(ow)
    vals = rng.integers(-10 ** 9, 10 ** 9, n).astype(np.int64)
    ok = (rng.random(n + OFF) >= 0.1).astype(np.uint8)
    valid = ctx.to_device(np.packbits(ok, bitorder="little"), pad=8)
    dvals = ctx.to_device(np.concatenate([np.zeros(OFF, np.int64), vals]))
    odt = np.int32 if ow == 4 else np.int64
    offs = ctx.alloc((n + 1) * ow)
    total = ctx.format_int_offsets(TYPE_IDS["int64"], dvals.ptr + OFF * 8, valid, OFF, n, ow, offs)
    texts = [str(v).encode() if ok[OFF + i] else b"" for i, v in enumerate(vals.tolist())]
    assert total == sum(map(len, texts))
    assert offs.download(odt, n + 1).tolist() == np.concatenate([[0], np.cumsum([len(t) for t in texts])]).tolist()
    guard = 32
    data = ctx.to_device(np.full(total + 2 * guard + 1, 0xAB, np.uint8))
    ctx.format_int_data(TYPE_IDS["int64"], dvals.ptr + OFF * 8, valid, OFF, n, ow, offs, data.ptr + guard + 1)   # an odd address: the stretch's ends are partial words
    raw = data.download(np.uint8, total + 2 * guard + 1).tobytes()
    assert raw[guard + 1:guard + 1 + total] == b"".join(texts)
    assert raw[:guard + 1] == b"\xab" * (guard + 1) and raw[guard + 1 + total:] == b"\xab" * guard      # nothing outside the stretch
    # the formatted column parsed back through ah_parse_int, then with offenders
    out = ctx.alloc(n * 8)
    rows = [t if t else b"bad!" for t in texts]                      # bytes under the nulls that would not parse
    host_offs = np.concatenate([[0], np.cumsum([len(t) for t in rows])]).astype(odt)
    doffs = ctx.to_device(np.concatenate([np.zeros(OFF, odt), host_offs]))
    ddata = ctx.to_device(np.frombuffer(b"".join(rows) + b"\0", np.uint8))
    ctx.parse_int(ow, doffs, ddata, valid, OFF, n, TYPE_IDS["int64"], out)
    assert out.download(np.int64, n).tolist() == [int(v) if ok[OFF + i] else 0 for i, v in enumerate(vals.tolist())]
    with pytest.raises(N.ErrInvalid) as e:
        ctx.parse_int(ow, doffs, ddata, None, OFF, n, TYPE_IDS["int64"], out)     # without the validity the bytes under the nulls count
    last_null = max(i for i in range(n) if not ok[OFF + i])
    assert (e.value.bad_row, e.value.bad_kind) == (last_null, 1)
    with pytest.raises(N.ErrInvalid) as e:
        ctx.parse_int(ow, doffs, ddata, valid, OFF, n, TYPE_IDS["int8"], out)
    last_big = max(i for i, v in enumerate(vals.tolist()) if ok[OFF + i] and not -128 <= v <= 127)
    assert (e.value.bad_row, e.value.bad_kind) == (last_big, 2)
    # utf8: the digits are ASCII; one row changed; fixed-size rows
    ctx.validate_utf8(ow, doffs, ddata, 0, valid, OFF, n)
    first_valid = [i for i in range(n) if ok[OFF + i]]
    bad_rows = sorted([first_valid[40], first_valid[300]])
    raw = bytearray(b"".join(rows))
    for r in bad_rows:
        raw[host_offs[r]] = 0xFF
    ddata.upload(np.frombuffer(bytes(raw), np.uint8))
    with pytest.raises(N.ErrInvalid) as e:
        ctx.validate_utf8(ow, doffs, ddata, 0, valid, OFF, n)
    assert e.value.bad_row == bad_rows[0]
    fixed = ctx.to_device(np.frombuffer(("é世" * 40).encode(), np.uint8))
    ctx.validate_utf8(0, None, fixed, 5, None, 2, 38)
    with pytest.raises(N.ErrInvalid) as e:
        ctx.validate_utf8(0, None, fixed, 4, None, 0, 50)
    assert e.value.bad_row == 0
    fo = ctx.alloc(8 * ow)
    ctx.fixed_binary_offsets(ow, 5, 2, 7, fo)
    assert fo.download(odt, 8).tolist() == [(2 + i) * 5 for i in range(8)]
    # booleans
    flags = rng.integers(0, 2, n + OFF).astype(np.uint8)
    dbits = ctx.to_device(np.packbits(flags, bitorder="little"), pad=8)
    total = ctx.format_int_offsets(1, dbits, valid, OFF, n, ow, offs)
    btexts = [(b"true" if flags[OFF + i] else b"false") if ok[OFF + i] else b"" for i in range(n)]
    assert total == sum(map(len, btexts))
    bdata = ctx.alloc(total + 8)
    ctx.format_int_data(1, dbits, valid, OFF, n, ow, offs, bdata)
    assert bdata.download(np.uint8, total).tobytes() == b"".join(btexts)
    pbits = ctx.to_device(np.full((n + 7) // 8 + 8, 0xFF, np.uint8))
    boffs = ctx.to_device(np.concatenate([np.zeros(OFF, odt), offs.download(odt, n + 1)]))
    ctx.parse_bool(ow, boffs, bdata, valid, OFF, n, pbits)
    got = np.unpackbits(pbits.download(np.uint8, (n + 7) // 8), bitorder="little")[:n].tolist()
    assert got == [int(flags[OFF + i]) if ok[OFF + i] else 0 for i in range(n)]
    assert pbits.download(np.uint8, (n + 7) // 8 + 8)[(n + 7) // 8:].tolist() == [0xFF] * 8        # nothing behind the bitmap
