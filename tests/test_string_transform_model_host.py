"""tests/string_transform_model.py against pyarrow (25.0.0 where this was written), for all thirteen functions over one fixed corpus:
empty rows, 1-byte rows, rows made only of trimmed characters, 2-, 3- and 4-byte code points at both ends, nulls, and all four types.
Only valid UTF-8 reaches pyarrow (it refuses anything else: "Invalid UTF8 sequence in input"); on other bytes the model is the
definition.  Also: pyarrow's offsets under nulls, and which input types pyarrow accepts that this project's table refuses."""
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from tests import string_transform_model as M

CORPUS = ["", "a", " ", "x", "  ", "xx", "xxxx", "ax", "xa", "xax", "héllo wörld", " héllo ", "\t\n x \r\v\f", " \t\n\r\v\f", "é", "éé", "€", "€uro€", "𝄞",
          "𝄞clef𝄞", "éa€b𝄞", "𝄞€é", "xxhéxx", "hé d", "ddd   hé", None, "abcdefghij" * 3, "é" * 7 + "€" * 5 + "𝄞" * 3, None, "A man, A PLAN: Ünïcode Zz@[`{"]
POSITIONS = (None, 0, 1, -1, 2, -2, 5, -5, 100, -100)
CHARACTER_SETS = ("", "x", " ", "hé d", "é€𝄞", " \t\n\r\v\f", "𝄞x")
STRING_TYPES = (pa.string(), pa.large_string())
BINARY_TYPES = (pa.binary(), pa.large_binary())
ROWS = [None if s is None else s.encode() for s in CORPUS]


def column(t):
    return pa.array(CORPUS if t in STRING_TYPES else ROWS, t)


def as_rows(arr):
    return [None if v is None else (v.encode() if isinstance(v, str) else bytes(v)) for v in arr.to_pylist()]


def offsets_of(arr):
    import numpy as np
    dtype = np.int64 if arr.type in (pa.large_string(), pa.large_binary()) else np.int32
    return np.frombuffer(arr.buffers()[1], dtype)[arr.offset:arr.offset + len(arr) + 1]


def check(got, want_rows, t, what):
    assert got.type == t, what
    assert as_rows(got) == want_rows, what
    assert got.null_count == sum(r is None for r in want_rows), what
    o = offsets_of(got)
    assert (o - o[0]).tolist() == M.offsets(want_rows).tolist(), (what, "offsets: a null row has length 0")


@pytest.mark.parametrize("t", STRING_TYPES, ids=str)
def test_case_mappings(t):
    check(pc.ascii_upper(column(t)), M.call("ascii_upper", ROWS), t, "ascii_upper")
    check(pc.ascii_lower(column(t)), M.call("ascii_lower", ROWS), t, "ascii_lower")
    assert M.call("ascii_upper", ["héllo".encode()]) == ["HéLLO".encode()]


@pytest.mark.parametrize("t", STRING_TYPES + BINARY_TYPES, ids=str)
def test_slices(t):
    name = "utf8_slice_codeunits" if t in STRING_TYPES else "binary_slice"
    fn = getattr(pc, name)
    for start in POSITIONS[1:]:
        for stop in POSITIONS:
            # pyarrow 25's binary_slice sizes its output from stop − start and answers "Negative buffer resize" to an absent stop
            # (INT64_MAX) behind a start ≥ 0: it is handed a stop beyond every row of the corpus instead, which slices the same
            pa_stop = 1 << 20 if stop is None and name == "binary_slice" and start >= 0 else stop
            check(fn(column(t), start, pa_stop), M.call(name, ROWS, start=start, stop=stop), t, (name, start, stop))


def test_the_checks_the_issue_names():
    s = "héllo wörld".encode()
    assert M.call("utf8_slice_codeunits", [s], start=-3, stop=-1) == [b"rl"]
    assert M.call("utf8_slice_codeunits", [s], start=-100, stop=2) == ["hé".encode()]
    assert M.call("utf8_slice_codeunits", [s], start=3, stop=1) == [b""]
    assert M.call("utf8_slice_codeunits", [b"ab"], start=2, stop=100) == [b""]
    assert M.call("utf8_trim", [s], chars="hé d".encode()) == ["llo wörl".encode()]
    got = pc.ascii_trim(pa.array(["xx", None, "ax"]), "x")
    assert offsets_of(got).tolist() == [0, 0, 0, 1] and got.null_count == 1
    assert M.offsets(M.call("ascii_trim", [b"xx", None, b"ax"], chars=b"x")).tolist() == [0, 0, 0, 1]


@pytest.mark.parametrize("t", STRING_TYPES, ids=str)
def test_trims(t):
    for side in ("trim", "ltrim", "rtrim"):
        name = f"ascii_{side}_whitespace"
        check(getattr(pc, name)(column(t)), M.call(name, ROWS), t, name)
        for chars in CHARACTER_SETS:
            for family in ("ascii", "utf8"):
                name = f"{family}_{side}"
                check(getattr(pc, name)(column(t), chars), M.call(name, ROWS, chars=chars.encode()), t, (name, chars))


def test_invalid_utf8_is_the_models_alone():
    """pyarrow refuses such input and is never handed any; the model's rule: the first byte of a row and every byte that is not
    10xxxxxx start a code point"""
    assert M.code_points(b"\x80\x80ab\xc3") == [b"\x80\x80", b"a", b"b", b"\xc3"]
    assert M.call("utf8_slice_codeunits", [b"a\x80\x80b\xe2\x82"], start=1, stop=None) == [b"b\xe2\x82"]
    assert M.call("utf8_slice_codeunits", [b"ab\x80"], start=-1, stop=None) == [b"b\x80"]
    assert M.call("utf8_rtrim", [b"ab\x80"], chars=b"b") == [b"ab\x80"]


def test_types_pyarrow_accepts_beyond_the_table():
    """The project's table: String / LargeString for twelve functions, Binary / LargeBinary for binary_slice.  What pyarrow takes
    beyond it is recorded here and listed in DESIGN.md §8 as left out."""
    candidates = {"string": pa.string(), "large_string": pa.large_string(), "binary": pa.binary(), "large_binary": pa.large_binary(),
                  "fixed_size_binary": pa.binary(2)}
    table = {name: ({"binary", "large_binary"} if name == "binary_slice" else {"string", "large_string"}) for name in M.FUNCTIONS}
    beyond = {}
    for name in M.FUNCTIONS:
        for tname, t in candidates.items():
            arr = pa.array(["ab", "cd"] if "string" in tname else [b"ab", b"cd"], t)
            options = pc.SliceOptions(0, 1) if name in M.SLICES else pc.TrimOptions("a") if name in M.TRIMS_WITH_CHARACTERS else None
            try:
                pc.call_function(name, [arr], options)
            except (pa.ArrowNotImplementedError, pa.ArrowInvalid, TypeError):
                assert tname not in table[name], (name, tname)
                continue
            if tname not in table[name]:
                beyond.setdefault(name, []).append(tname)
    assert beyond == {"binary_slice": ["fixed_size_binary"]}
