"""The conversion rules of the string casts (csrc/ah_strconv.h) on the CPU: the header compiled for the host against
tests/strconv_model.py (Go's ParseInt / ParseUint / ParseBool restated) and Python itself (str(v), bytes.decode("utf-8")).  The
restatement is pinned first by the reference's own vectors (TestStringToInt, compute/cast_test.go:2542-2579).  The harness hands every
row to the header in an allocation of exactly the row's size."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

from tests import strconv_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"]
KIND = {0: None, 1: M.SYNTAX, 2: M.RANGE}


@pytest.fixture(scope="module")
def host():
    d = tempfile.mkdtemp(prefix="strconvh_")
    so = os.path.join(d, "libstrconvh.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", os.path.join(ROOT, "tests", "strconv_harness.cc"), "-o", so])
    lib = C.CDLL(so)
    vp, lg, it = C.c_void_p, C.c_long, C.c_int
    lib.sh_parse_int.argtypes = [vp, vp, lg, it, it, vp, vp]
    lib.sh_parse_bool.argtypes = [vp, vp, lg, vp, vp]
    lib.sh_format_int.argtypes = [vp, lg, it, vp, vp]
    lib.sh_format_bool.argtypes = [it, vp, vp]
    lib.sh_utf8_valid.argtypes = [vp, vp, lg, lg, vp]
    for f in (lib.sh_parse_int, lib.sh_parse_bool, lib.sh_format_int, lib.sh_format_bool, lib.sh_utf8_valid):
        f.restype = None
    return lib


def column(rows):
    """(data, int64 offsets) of a list of byte strings; one spare byte so that an empty column still has an address"""
    offsets = np.zeros(len(rows) + 1, np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    data = np.frombuffer(b"".join(rows) + b"\0", np.uint8).copy()
    return data, offsets


def parse_int(host, type_name, rows):
    data, offsets = column(rows)
    values, kinds = np.zeros(len(rows), np.uint64), np.zeros(len(rows), np.uint8)
    host.sh_parse_int(data.ctypes.data, offsets.ctypes.data, len(rows), M.INT_BITS[type_name], int(not type_name.startswith("u")),
                      values.ctypes.data, kinds.ctypes.data)
    bits = M.INT_BITS[type_name]
    out = []
    for v, k in zip(values.tolist(), kinds.tolist()):
        if k:
            out.append((None, KIND[k]))
        else:
            if not type_name.startswith("u") and v >> 63:   # a signed value comes sign-extended to 64 bits
                v -= 1 << 64
            out.append((v, None))
    return out


def test_the_restatement_agrees_with_the_reference_vectors():
    for t, s, v in M.GOLDEN_ACCEPTED:
        assert M.go_parse(t, s) == (v, None), (t, s)
    want = dict(zip(M.GOLDEN_NOT_INT8, [M.SYNTAX, M.SYNTAX, M.RANGE, M.RANGE, M.SYNTAX, M.SYNTAX, M.RANGE, M.RANGE]))
    for s in M.GOLDEN_NOT_INT8:
        assert M.go_parse("int8", s) == (None, want[s]), s
    want = dict(zip(M.GOLDEN_NOT_UINT8, [M.RANGE, M.SYNTAX, M.SYNTAX, M.SYNTAX, M.SYNTAX, M.RANGE]))
    for s in M.GOLDEN_NOT_UINT8:
        assert M.go_parse("uint8", s) == (None, want[s]), s
    # the points where Python's int(s, 0) and Go part
    assert M.go_parse("int32", b"012") == (10, None) and M.go_parse("int32", b" 1") == (None, M.SYNTAX)
    assert M.go_parse("int32", b"0_7") == (7, None) and M.go_parse("int32", b"0x_1") == (1, None)
    assert M.go_parse("int32", b"1__2") == (None, M.SYNTAX) and M.go_parse("int32", b"08") == (None, M.SYNTAX)
    assert M.go_parse("int8", b"1" * 25 + b"z") == (None, M.RANGE)
    assert M.parse_error_text("int8", b"12 z", M.SYNTAX) == 'strconv.ParseInt: parsing "12 z": invalid syntax'
    assert M.parse_error_text("uint8", b"256", M.RANGE) == 'strconv.ParseUint: parsing "256": value out of range'
    assert M.parse_error_text("bool", b"yes", M.SYNTAX) == 'strconv.ParseBool: parsing "yes": invalid syntax'


def in_base(v, base, upper):
    """v with Go's base prefix, the prefix letter and the digits in one case"""
    digits = {2: "{:b}", 8: "{:o}", 10: "{:d}", 16: "{:x}"}[base].format(abs(v))
    prefix = {2: "0b", 8: "0o", 10: "", 16: "0x"}[base]
    text = ("-" if v < 0 else "") + (prefix + digits).upper() if upper else ("-" if v < 0 else "") + prefix + digits
    return text.encode()


def parse_rows(type_name, rng):
    bits = M.INT_BITS[type_name]
    lo, hi = (0, (1 << bits) - 1) if type_name.startswith("u") else (-(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    rows = [s for t, s, _ in M.GOLDEN_ACCEPTED if t == type_name] + M.GOLDEN_NOT_INT8 + M.GOLDEN_NOT_UINT8
    for v in (lo, hi, lo - 1, hi + 1):
        for base in (2, 8, 10, 16):
            for upper in (False, True):
                rows.append(in_base(v, base, upper))
        rows.append(b"0" + "{:o}".format(abs(v)).encode() if v >= 0 else b"-0" + "{:o}".format(abs(v)).encode())   # the bare octal 0
    rows += [b"", b"+", b"-", b"0", b"-0", b"+0", b"00", b"08", b"0_7", b"0x_1", b"1__2", b"_1", b"1_", b"0b102", b" 1", b"1 ",
             b"1" * 25 + b"z", b"+1", b"-1", b"0x", b"0X", b"0b", b"0o", b"0o7", b"0O17", b"0b1_0", b"1_000", b"0_", b"0x1_", b"-_1",
             b"9" * 19, b"9" * 20, b"9" * 21 + b"_", b"0x" + b"f" * 17 + b" ", b"1" * 300, b"0" * 299 + b"7", b"0" * 64 + b"9"]
    alphabet = b"0123456789abcdefxXbo_+-z"
    for _ in range(4000):
        rows.append(bytes(rng.choice(alphabet) for _ in range(rng.randint(0, 24))))
    for _ in range(1000):   # strings that are mostly numbers of about the right size
        v = rng.randint(lo * 2 - 2, hi * 2 + 2)
        s = in_base(v, rng.choice((2, 8, 10, 16)), rng.random() < 0.5)
        if rng.random() < 0.3 and len(s) > 1:
            at = rng.randint(0, len(s))
            s = s[:at] + rng.choice([b"_", b"z", b" ", b"+"]) + s[at:]
        rows.append(s)
    return rows


@pytest.mark.parametrize("type_name", TYPES)
def test_parse_integer_matches_the_restatement(host, type_name):
    rows = parse_rows(type_name, random.Random(100 + TYPES.index(type_name)))
    got = parse_int(host, type_name, rows)
    bad = 0
    for s, g in zip(rows, got):
        want = M.go_parse(type_name, s)
        assert g == want, (type_name, s, g, want)
        if want[1]:
            bad += 1
            fn = "ParseUint" if type_name.startswith("u") else "ParseInt"
            assert M.parse_error_text(type_name, s, g[1]) == "strconv.%s: parsing %s: %s" % (fn, M.go_quote_ascii(s), want[1])
    assert 0 < bad < len(rows)


def test_parse_integer_golden_vectors(host):
    for t in TYPES:
        acc = [(s, v) for tt, s, v in M.GOLDEN_ACCEPTED if tt == t]
        assert parse_int(host, t, [s for s, _ in acc]) == [(v, None) for _, v in acc], t
    assert [k for _, k in parse_int(host, "int8", M.GOLDEN_NOT_INT8)] == [M.SYNTAX, M.SYNTAX, M.RANGE, M.RANGE, M.SYNTAX, M.SYNTAX, M.RANGE, M.RANGE]
    assert [k for _, k in parse_int(host, "uint8", M.GOLDEN_NOT_UINT8)] == [M.RANGE, M.SYNTAX, M.SYNTAX, M.SYNTAX, M.SYNTAX, M.RANGE]


def test_parse_bool(host):
    rows = M.TRUE_SPELLINGS + M.FALSE_SPELLINGS + [b"", b"TRUE ", b"tRUE", b"yes", b"2", b"tru", b"truee", b"fals", b"falsey", b"FALSe", b"T\0", b"true\0\0"]
    data, offsets = column(rows)
    values, kinds = np.zeros(len(rows), np.uint8), np.zeros(len(rows), np.uint8)
    host.sh_parse_bool(data.ctypes.data, offsets.ctypes.data, len(rows), values.ctypes.data, kinds.ctypes.data)
    for s, v, k in zip(rows, values.tolist(), kinds.tolist()):
        want, err = M.go_parse_bool(s)
        assert KIND[k] == err and (err or bool(v) == want), (s, v, k)
        if err:
            assert v == 0
    assert sum(kinds.tolist()) == len(rows) - 12


@pytest.mark.parametrize("type_name", TYPES)
def test_format_integer_matches_str(host, type_name):
    bits = M.INT_BITS[type_name]
    signed = not type_name.startswith("u")
    lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
    rng = random.Random(bits + signed)
    vals = {lo, hi, 0, 1, -1}
    for p in range(0, 21):
        vals |= {10 ** p, 10 ** p - 1, -(10 ** p), -(10 ** p) + 1, -(10 ** p) - 1}
    vals = sorted(v for v in vals if lo <= v <= hi) + [rng.randint(lo, hi) for _ in range(3000)] + [rng.randint(-99999, 99999) for _ in range(500)]
    vals = [v for v in vals if lo <= v <= hi]
    patterns = np.array([v & ((1 << 64) - 1) for v in vals], np.uint64)   # sign-extended to 64 bits
    lens, chars = np.zeros(len(vals), np.int32), np.zeros(len(vals) * 20, np.uint8)
    host.sh_format_int(patterns.ctypes.data, len(vals), int(signed), lens.ctypes.data, chars.ctypes.data)
    raw = chars.tobytes()
    for i, v in enumerate(vals):
        assert lens[i] == len(str(v)), v
        assert raw[i * 20:i * 20 + lens[i]] == str(v).encode(), v
        assert raw[i * 20 + lens[i]:(i + 1) * 20] == b"\0" * (20 - lens[i]), v   # nothing written behind the last character


def test_format_bool(host):
    for v, text in ((1, b"true"), (0, b"false")):
        n, chars = C.c_int(0), np.zeros(8, np.uint8)
        host.sh_format_bool(v, C.byref(n), chars.ctypes.data)
        assert n.value == len(text) and chars.tobytes()[:n.value] == text and chars.tobytes()[n.value:] == b"\0" * (8 - n.value)


def py_valid(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def utf8_rows(rng):
    rows = [chr(cp).encode("utf-8") for cp in (0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000, 0x10FFFF, 0xD7FF, 0xE000)]
    rows += [b"\xC0\x80", b"\xE0\x80\x80", b"\xED\xA0\x80", b"\xED\xBF\xBF", b"\xF4\x90\x80\x80", b"\x80", b"\xBF", b"\xC1\xBF", b"\xF5\x80\x80\x80",
             b"\xFF", b"\xF0\x8F\xBF\xBF", b"\xE0\x9F\xBF", b"", b"a", b"\xa0\xa1", b"Hi", "olá mundo".encode(), "你好世界".encode()]
    four = "\U0001F600".encode("utf-8")
    rows += [four[:k] for k in range(1, 4)] + [b"abc" + four[:k] for k in range(1, 4)] + [four[:k] + b"a" for k in range(1, 4)]
    three = "世".encode("utf-8")
    # a sequence across every position of an 8-byte word, whole and cut short, and a stray continuation byte behind ASCII
    for pad in range(0, 18):
        for seq in (three, four, "é".encode("utf-8")):
            rows += [b"a" * pad + seq + b"b" * 9, b"a" * pad + seq, b"a" * pad + seq[:-1], b"a" * pad + seq[:-1] + b"b" * 9, b"a" * pad + seq[1:] + b"b" * 3]
    text = ("añ世\U0001F600z" * 70).encode("utf-8")
    rows += [text, text[:-1], text[:-2], text[1:], text[2:]]
    for _ in range(3000):
        rows.append(bytes(rng.getrandbits(8) for _ in range(rng.randint(0, 40))))
    for _ in range(2000):   # valid text with at most one byte changed
        s = "".join(chr(rng.choice([rng.randint(0, 0x7F), rng.randint(0x80, 0x7FF), rng.randint(0x800, 0xD7FF), rng.randint(0xE000, 0xFFFF),
                                    rng.randint(0x10000, 0x10FFFF)])) for _ in range(rng.randint(0, 20))).encode("utf-8")
        if s and rng.random() < 0.6:
            at = rng.randrange(len(s))
            s = s[:at] + bytes([rng.getrandbits(8)]) + s[at + 1:]
        rows.append(s)
    return rows


@pytest.mark.parametrize("piece", [0, 1, 3, 8, 16, 64])
def test_utf8_valid_matches_python(host, piece):
    """piece 0: the whole row; else the row validated in pieces of that many bytes, as the kernel's whole-wave path cuts a long row"""
    rows = utf8_rows(random.Random(7))
    data, offsets = column(rows)
    ok = np.zeros(len(rows), np.uint8)
    host.sh_utf8_valid(data.ctypes.data, offsets.ctypes.data, len(rows), piece, ok.ctypes.data)
    want = [py_valid(r) for r in rows]
    for r, g, w in zip(rows, ok.tolist(), want):
        assert bool(g) == w, (piece, r)
    assert 0 < sum(want) < len(rows)
