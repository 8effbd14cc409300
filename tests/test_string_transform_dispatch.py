"""The string transforms in the function registry, resolved without a device: the thirteen names and their kernel counts, the types
each accepts and refuses (with the registry's usual dispatch error), the output type = the input type, and what the functions answer
to their options string.  (The two C entry points are libarrowhip.so's: tests/test_string_match_dispatch.py holds the header check.)"""
import pytest

from arrow_go_amd import compute as ac
from tests.test_string_match_dispatch import dispatch_ids

STRING, BINARY, LARGE_STRING, LARGE_BINARY, FSB, INT32, BOOL = 13, 14, 34, 35, 15, 7, 1   # arrow.Type ids
STRING_FNS = ("ascii_upper", "ascii_lower", "utf8_slice_codeunits", "ascii_trim", "ascii_ltrim", "ascii_rtrim", "ascii_trim_whitespace",
              "ascii_ltrim_whitespace", "ascii_rtrim_whitespace", "utf8_trim", "utf8_ltrim", "utf8_rtrim")
NAMES = STRING_FNS + ("binary_slice",)
SLICES = ("utf8_slice_codeunits", "binary_slice")
CHARACTER_TRIMS = ("ascii_trim", "ascii_ltrim", "ascii_rtrim", "utf8_trim", "utf8_ltrim", "utf8_rtrim")


def accepted(name):
    return (BINARY, LARGE_BINARY) if name == "binary_slice" else (STRING, LARGE_STRING)


def test_the_thirteen_functions_are_registered():
    assert len(NAMES) == 13
    for name in NAMES:
        assert ac.has_function(name), name
        assert ac.function_num_kernels(name) == 2, name
    for wrong in ("replace_substring", "utf8_lower", "utf8_upper", "utf8_trim_whitespace", "binary_join_element_wise", "utf8_slice", "ascii_trim_left"):
        assert not ac.has_function(wrong), wrong


def test_accepted_types_dispatch_exactly_and_come_back():
    for name in NAMES:
        for t in accepted(name):
            assert dispatch_ids(name, [t]) == [t]
            assert ac.output_type_id(name, [t]) == t


def test_refusals():
    for name in NAMES:
        refused = {STRING: "utf8", LARGE_STRING: "large_utf8", BINARY: "binary", LARGE_BINARY: "large_binary"}
        for t in accepted(name):
            del refused[t]
        for t in refused:
            with pytest.raises(ac.ErrNotImplemented, match=rf"function '{name}' has no kernel matching input types \("):
                dispatch_ids(name, [t])
        for t, shown in ((INT32, "int32"), (BOOL, "bool")):
            with pytest.raises(ac.ErrNotImplemented, match=rf"function '{name}' has no kernel matching input types \({shown}\)"):
                dispatch_ids(name, [t])
        with pytest.raises(ac.ErrNotImplemented, match=rf"function '{name}' has no kernel matching input types"):
            dispatch_ids(name, [FSB])
        with pytest.raises(ac.ErrInvalid, match=rf"function '{name}' accepts 1 arguments but 2 passed"):
            dispatch_ids(name, [accepted(name)[0]] * 2)


def test_slice_options():
    for name in SLICES:
        for good in ("start=0", "start=-5;stop=7", "stop=-1;start=+3", "start=2;stop=1;step=1", "start=-9223372036854775808;stop=9223372036854775807"):
            ac.validate_options(name, good)
        with pytest.raises(ac.ErrInvalid, match=rf"function '{name}' needs the option start=<int64>"):
            ac.validate_options(name, "")
        with pytest.raises(ac.ErrInvalid, match="needs the option start"):
            ac.validate_options(name, "stop=3")
        for bad, key in (("start=a", "start"), ("start=1.5", "start"), ("start=", "start"), ("start=1;stop=0x10", "stop"), ("start=1;step=two", "step"),
                         ("start=9223372036854775808", "start"), ("start=int64:1", "start")):
            with pytest.raises(ac.ErrInvalid, match=rf"function '{name}': {key} is not an int64"):
                ac.validate_options(name, bad)
        for step in (2, -1, 3):
            with pytest.raises(ac.ErrNotImplemented, match=rf"step={step} is not implemented"):
                ac.validate_options(name, f"start=0;step={step}")
        with pytest.raises(ac.ErrInvalid, match="step cannot be zero"):
            ac.validate_options(name, "start=0;step=0")
    assert ac.slice_options(1) == "start=1" and ac.slice_options(-2, 5) == "start=-2;stop=5" and ac.slice_options(0, None, -1) == "start=0;step=-1"
    ac.validate_options("cumulative_sum", "start=int64:10")   # the cumulative functions' key of the same name is untouched


def test_trim_options():
    for name in CHARACTER_TRIMS:
        for good in ("characters_hex=", "characters_hex=20", "characters_hex=3b3d00", "characters_hex=c3a9e282acf09d849e", "characters_hex=" + "61" * 1024):
            ac.validate_options(name, good)
        ac.validate_options(name, ac.trim_options("hé d"))
        with pytest.raises(ac.ErrInvalid, match=rf"function '{name}' needs the option characters_hex"):
            ac.validate_options(name, "")
        for bad in ("6", "6g", "0x61", "61 62", "616"):
            with pytest.raises(ac.ErrInvalid, match="characters_hex is not a string of hex byte pairs"):
                ac.validate_options(name, "characters_hex=" + bad)
        with pytest.raises(ac.ErrNotImplemented, match="at most 1024"):
            ac.validate_options(name, "characters_hex=" + "61" * 1025)
    for bad in ("ff", "c3", "80", "e282", "c0af", "eda080", "f4908080"):   # stray, truncated, overlong, a surrogate, above U+10FFFF
        for name in ("utf8_trim", "utf8_ltrim", "utf8_rtrim"):
            with pytest.raises(ac.ErrInvalid, match="the characters are not valid UTF-8"):
                ac.validate_options(name, "characters_hex=" + bad)
        for name in ("ascii_trim", "ascii_ltrim", "ascii_rtrim"):
            ac.validate_options(name, "characters_hex=" + bad)   # a set of bytes: any bytes
    for name in ("ascii_upper", "ascii_lower", "ascii_trim_whitespace", "ascii_ltrim_whitespace", "ascii_rtrim_whitespace"):
        ac.validate_options(name, "")
    assert ac.trim_options("a;=") == "characters_hex=613b3d" and ac.trim_options(b"\xff\x00") == "characters_hex=ff00" and ac.trim_options("") == "characters_hex="
