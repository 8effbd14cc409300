"""The string predicates in the function registry, resolved without a device: the seven names, the types each accepts and refuses
(with the registry's usual dispatch error), the output type per input type, and what the pattern functions answer to their options
string.  The six string entry points (these predicates and the transforms) are libarrowhip.so's, declared in a header of their
own, include/arrowhip_strings.h: header ⊆ nm -D and both headers == nm -D are checked here."""
import ctypes as C
import os

import pyarrow as pa
import pytest

from arrow_go_amd import _native as N
from arrow_go_amd import compute as ac

PATTERN_FNS = ("match_substring", "starts_with", "ends_with", "find_substring", "match_like")
NAMES = PATTERN_FNS + ("binary_length", "utf8_length")
STRING, BINARY, LARGE_STRING, LARGE_BINARY, FSB, INT32, INT64, BOOL = 13, 14, 34, 35, 15, 7, 9, 1   # arrow.Type ids
BINARY_LIKE = (STRING, BINARY, LARGE_STRING, LARGE_BINARY)


def dispatch_ids(name, ids):
    """ahc_dispatch_best over raw type ids (compute.dispatch_best has no spelling for FixedSizeBinary)"""
    n = len(ids)
    out = (C.c_int * n)()
    err = C.create_string_buffer(1024)
    rc = ac.lib.ahc_dispatch_best(name.encode(), n, (C.c_int * n)(*ids), out, err, len(err))
    if rc != 0:
        raise ac._ERRS.get(rc, ac.ArrowError)(err.value.decode(errors="replace"))
    return list(out)


def test_the_seven_functions_are_registered():
    for name in NAMES:
        assert ac.lib.ahc_has_function(name.encode()), name
    assert [ac.function_num_kernels(n) for n in NAMES] == [4, 4, 4, 4, 4, 5, 2]
    for wrong in ("match_substring_regex", "count_substring", "find_substring_regex", "utf8_upper", "binary_len"):
        assert not ac.has_function(wrong)


def test_the_string_header_is_exported_by_the_one_library():
    """include/arrowhip_strings.h declares the six string entry points; libarrowhip.so exports every one of them, and exports exactly
    what include/arrowhip.h and include/arrowhip_strings.h declare together"""
    import subprocess
    declared = N.declared_symbols(N.STRINGS_HEADER_PATH)
    assert declared == ["ah_string_find", "ah_string_gather", "ah_string_length", "ah_string_like", "ah_string_match", "ah_string_ranges"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = sorted(l.split()[-1] for l in out.splitlines() if " T " in l)
    assert set(declared) <= set(exported)
    assert exported == sorted(set(N.declared_symbols(N.HEADER_PATH)) | set(declared))
    assert not set(declared) & set(N.declared_symbols(N.HEADER_PATH))   # (the Go shim binds include/arrowhip.h entry for entry)
    src = '#include "arrowhip_strings.h"\nint main(void) { return 0; }\n'   # plain C11, like the other two boundary headers
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.dirname(N.STRINGS_HEADER_PATH), "-x", "c", "-"],
                   input=src, text=True, check=True)


def test_accepted_types_dispatch_exactly():
    for name in PATTERN_FNS + ("binary_length",):
        for t in BINARY_LIKE:
            assert dispatch_ids(name, [t]) == [t]
    assert dispatch_ids("binary_length", [FSB]) == [FSB]
    for t in (STRING, LARGE_STRING):
        assert dispatch_ids("utf8_length", [t]) == [t]
    for t in (pa.string(), pa.binary(), pa.large_string(), pa.large_binary()):
        assert ac.dispatch_best("match_like", [t]) == [t]


def test_output_types():
    for t in BINARY_LIKE:
        wide = INT64 if t in (LARGE_STRING, LARGE_BINARY) else INT32
        for name in ("match_substring", "starts_with", "ends_with", "match_like"):
            assert ac.output_type_id(name, [t]) == BOOL
        assert ac.output_type_id("find_substring", [t]) == wide
        assert ac.output_type_id("binary_length", [t]) == wide
    assert ac.output_type_id("binary_length", [FSB]) == INT32
    assert ac.output_type_id("utf8_length", [STRING]) == INT32 and ac.output_type_id("utf8_length", [LARGE_STRING]) == INT64
    assert ac.output_type_id("add", [INT32, INT32]) == INT32 and ac.output_type_id("equal", [STRING, STRING]) == BOOL   # (the export itself)


def test_refusals():
    for name in NAMES:
        with pytest.raises(ac.ErrNotImplemented, match=rf"function '{name}' has no kernel matching input types \(int32\)"):
            dispatch_ids(name, [INT32])
        with pytest.raises(ac.ErrNotImplemented, match=rf"function '{name}' has no kernel matching input types \(bool\)"):
            dispatch_ids(name, [BOOL])
        with pytest.raises(ac.ErrInvalid, match=rf"function '{name}' accepts 1 arguments but 2 passed"):
            dispatch_ids(name, [STRING, STRING])
    for name in PATTERN_FNS + ("utf8_length",):
        with pytest.raises(ac.ErrNotImplemented, match=rf"function '{name}' has no kernel matching input types"):
            dispatch_ids(name, [FSB])
    for t in (BINARY, LARGE_BINARY):
        with pytest.raises(ac.ErrNotImplemented, match=r"function 'utf8_length' has no kernel matching input types \((large_)?binary\)"):
            dispatch_ids("utf8_length", [t])


def test_options():
    for name in PATTERN_FNS:
        ac.validate_options(name, "pattern_hex=")                       # the empty pattern is a pattern
        ac.validate_options(name, "pattern_hex=3b3dff00")               # ';', '=', a byte that is no UTF-8, a zero byte
        ac.validate_options(name, "pattern_hex=61;ignore_case=false")
        ac.validate_options(name, ac.pattern_options("a;=é"))
        with pytest.raises(ac.ErrInvalid, match=rf"function '{name}' needs the option pattern_hex"):
            ac.validate_options(name, "")
        with pytest.raises(ac.ErrInvalid, match="needs the option pattern_hex"):
            ac.validate_options(name, "ignore_case=false")
        for bad in ("6", "6g", "0x61", "61 62"):
            with pytest.raises(ac.ErrInvalid, match="pattern_hex is not a string of hex byte pairs"):
                ac.validate_options(name, "pattern_hex=" + bad)
        with pytest.raises(ac.ErrNotImplemented, match="ignore_case=true is not implemented"):
            ac.validate_options(name, "pattern_hex=61;ignore_case=true")
        with pytest.raises(ac.ErrNotImplemented, match="at most 4096"):
            ac.validate_options(name, "pattern_hex=" + "61" * 4097)
    ac.validate_options("binary_length", "")
    ac.validate_options("utf8_length", "")
    with pytest.raises(ac.ErrKey):
        ac.validate_options("match_substring_regex", "pattern_hex=61")
    assert ac.pattern_options("a;=") == "pattern_hex=613b3d" and ac.pattern_options(b"\xff", ignore_case=True) == "pattern_hex=ff;ignore_case=true"
