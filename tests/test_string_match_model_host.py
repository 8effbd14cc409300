"""The host model of the string predicates (tests/string_match_model.py) pinned to pyarrow, and the host-side LIKE compiler
(arrow_go_amd/host/like_program.h through ahc_like_compile) checked against the same model through a small interpreter — all
without a device.  Expected values are exact everywhere."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from arrow_go_amd import compute as ac
from tests import string_match_model as M

TYPES = [pa.string(), pa.binary(), pa.large_string(), pa.large_binary()]
LIKE_PATTERNS = ["%", "%%", "_", "a%", "%a", "%a%b%", "a_c", "_%_", "\\%", "\\_", "a\\", "", "%é_", "a%%b", "__", "%_%_%", "_%", "%__", "a%b", "ab",
                 "%ab", "ab%", "%ab%", "a\\%c", "a\\bc", "%\\\\%", "é", "%a\\bc%", "a\\bc%", "%a\\bc", "%a\\", "%\\", "a%\\", "\\", "a\\%%", "%a\\%", "_é%", "%b_", "a_%_c", "%a_c%b", "x" * 50, "%" + "ab" * 30 + "%"]
ALPHABET = ["a", "b", "c", "ab", "%", "_", "\\", "é", "\n", "日", "x", ""]


def random_texts(rng, n, max_pieces=8):
    return ["".join(rng.choice(ALPHABET, rng.integers(0, max_pieces + 1))) for _ in range(n)]


def column(rng, n=300):
    texts = random_texts(rng, n) + ["", "a", "ab", "abc", "a%c", "a\\", "a_c", "aéc", "héllo\nx", "h_llo", "abab", "aaaa", "b" * 40, "ab" * 30, "ab" * 30 + "c"]
    valid = rng.random(len(texts)) < 0.85
    return texts, valid


def as_array(texts, valid, t):
    vals = [x if v else None for x, v in zip(texts, valid)]
    if pa.types.is_binary(t) or pa.types.is_large_binary(t):
        vals = [None if x is None else x.encode() for x in vals]
    return pa.array(vals, type=t)


def is_utf8(t):
    return pa.types.is_string(t) or pa.types.is_large_string(t)


def check(model_values, arrow_result, valid, what):
    got = arrow_result.to_pylist()
    for i, ok in enumerate(valid):
        if ok:
            assert got[i] == model_values[i], (what, i)
        else:
            assert got[i] is None, (what, i)


@pytest.mark.parametrize("t", TYPES, ids=str)
def test_substring_family_is_pyarrows(t):
    rng = np.random.default_rng(11)
    texts, valid = column(rng)
    arr = as_array(texts, valid, t)
    rows = [x.encode() for x in texts]
    for pat in ["", "a", "ab", "abc", "é", "\n", "aa", "abab", "b" * 40, "b" * 41, "ab" * 30 + "c", "ab" * 31]:
        p = pat.encode()
        check(M.match_substring(rows, p).tolist(), pc.match_substring(arr, pat), valid, ("match_substring", pat))
        check(M.starts_with(rows, p).tolist(), pc.starts_with(arr, pat), valid, ("starts_with", pat))
        check(M.ends_with(rows, p).tolist(), pc.ends_with(arr, pat), valid, ("ends_with", pat))
        check(M.find_substring(rows, p).tolist(), pc.find_substring(arr, pat), valid, ("find_substring", pat))
    want_find = pa.int64() if "large" in str(t) else pa.int32()
    assert pc.find_substring(arr, "a").type == want_find and pc.binary_length(arr).type == want_find
    check(M.binary_length(rows).tolist(), pc.binary_length(arr), valid, "binary_length")
    if is_utf8(t):
        check(M.utf8_length(rows).tolist(), pc.utf8_length(arr), valid, "utf8_length")
        assert pc.utf8_length(arr).type == want_find


def test_binary_length_of_fixed_size_binary():
    arr = pa.array([b"abc", None, b"xyz"], type=pa.binary(3))
    assert pc.binary_length(arr).to_pylist() == [3, None, 3] and pc.binary_length(arr).type == pa.int32()


@pytest.mark.parametrize("t", TYPES, ids=str)
def test_like_model_is_pyarrows(t):
    rng = np.random.default_rng(12)
    texts, valid = column(rng)
    arr = as_array(texts, valid, t)
    rows = [x.encode() for x in texts]
    for pat in LIKE_PATTERNS:
        check(M.match_like(rows, pat.encode(), is_utf8(t)).tolist(), pc.match_like(arr, pat), valid, ("match_like", pat))


def test_like_rules_checked_by_hand():
    assert M.match_like([b"h\xc3\xa9llo\nx", b"h_llo"], b"h_llo%", True).tolist() == [True, True]
    assert M.match_like([b"a%c", b"abc", b"a\\%c"], b"a\\%c", True).tolist() == [True, False, False]
    assert M.match_like([b"ab", b"a\\b"], b"a\\b", True).tolist() == [True, False]
    # a lone escape character at the end: pyarrow 25 drops it (its regular expression is built character by character and the pending
    # escape is never written), so `a\` is the pattern `a` — it does not match the row `a\`, and it is not "nothing" either
    assert M.match_like([b"a\\", b"a"], b"a\\", True).tolist() == [False, True]
    assert pc.match_like(pa.array(["a\\", "a"]), "a\\").to_pylist() == [False, True]
    # Arrow's substring / prefix / suffix shortcuts take what stands between the `%` raw, backslashes included
    assert M.match_like([b"abc", b"xa\\bcx"], b"%a\\bc%", True).tolist() == [False, True]
    assert pc.match_like(pa.array(["abc", "xa\\bcx"]), "%a\\bc%").to_pylist() == [False, True]
    assert M.match_like([b"a\\", b"a"], b"%a\\", True).tolist() == [True, False]
    assert pc.match_like(pa.array(["a\\", "a"]), "%a\\").to_pylist() == [True, False]
    assert M.match_like([b"h\xffllo"], b"h_llo", False).tolist() == [True]
    assert M.match_like([b"h\xc3\xa9llo"], b"h_llo", False).tolist() == [False]   # two bytes are two characters of a Binary row


def test_like_compiler_programs():
    assert ac.like_compile("%") == bytes([0, 0, 0]) == ac.like_compile("%%")
    assert ac.like_compile("") == bytes([3, 1, 0, 0, 0])
    assert ac.like_compile("a%") == bytes([1, 1, 0, 1, 0, 0, ord("a")])
    assert ac.like_compile("%a") == bytes([2, 1, 0, 1, 0, 0, ord("a")])
    assert ac.like_compile("%a%b%") == bytes([0, 2, 0, 1, 0, 0, ord("a"), 1, 0, 0, ord("b")])
    assert ac.like_compile("a_c") == bytes([3, 1, 0, 3, 0, 0, ord("a"), 1, 0, 0, ord("c")])
    assert ac.like_compile("\\%") == bytes([3, 1, 0, 1, 0, 0, ord("%")])
    assert ac.like_compile("a\\") == ac.like_compile("a")           # the lone escape character at the end is dropped
    assert ac.like_compile("%a\\") == bytes([2, 1, 0, 2, 0, 0, ord("a"), 0, ord("\\")])   # the suffix shortcut: raw
    assert ac.like_compile("%a\\b%") == bytes([0, 1, 0, 3, 0, 0, ord("a"), 0, ord("\\"), 0, ord("b")])
    assert ac.like_compile("a\\b") == ac.like_compile("ab")
    assert ac.like_compile("a%%b") == ac.like_compile("a%b")


def test_like_compiler_under_sanitizers():
    """the header-only compiler as a stand-alone program (tests/like_program_harness.cc) under AddressSanitizer and UBSan: the same
    programs as the library's export, and nothing for the sanitizers to report"""
    import os
    import shutil
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    d = tempfile.mkdtemp(prefix="like_program_harness_")
    try:
        exe = os.path.join(d, "like_program_harness")
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                            os.path.join(root, "tests", "like_program_harness.cc")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        rng = np.random.default_rng(14)
        pats = [p.encode() for p in LIKE_PATTERNS] + [bytes(rng.choice(np.frombuffer(b"ab%_\\\xc3\xa9", np.uint8), int(k))) for k in rng.integers(0, 12, 400)]
        pats += [b"%" * 300, b"_" * 300, b"\\" * 301, b"a%" * 600, b"\\%" * 200 + b"\\"]
        p = subprocess.run([exe], input="\n".join(x.hex() or "-" for x in pats) + "\n", capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and not p.stderr, f"exit {p.returncode}\n{p.stderr[-3000:]}"
        out = p.stdout.splitlines()
        assert len(out) == len(pats)
        for pat, line in zip(pats, out):
            assert bytes.fromhex(line) == ac.like_compile(pat), pat
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("utf8", [True, False])
def test_compiled_programs_match_the_model(utf8):
    rng = np.random.default_rng(13)
    texts, _ = column(rng, 400)
    rows = [x.encode() for x in texts]
    if not utf8:
        rows += [b"h\xffllo", b"\x80\x80", b"a\xc3", b"\xa9c"]
    extra = ["".join(rng.choice(["a", "b", "%", "_", "\\", "é", "%%"], rng.integers(0, 7))) for _ in range(150)]
    for pat in LIKE_PATTERNS + extra:
        program = ac.like_compile(pat)
        want = M.match_like(rows, pat.encode(), utf8).tolist()
        got = [M.run_program(program, r, utf8) for r in rows]
        assert got == want, (pat, [r for r, g, w in zip(rows, got, want) if g != w][:3])
