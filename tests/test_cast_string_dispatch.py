"""The string casts in the host layer's registry, on a machine without a GPU: the five cast functions the reference registers for
binary-like targets (compute/cast.go:906-912), their kernels (GetToBinaryKernels / GetFsbCastKernels, kernels/string_casts.go:224-256,
581-607), and the String / Binary input kernels of the integer and boolean casts (numeric_cast.go:815-833, boolean_cast.go:77-95),
which sit beside each function's numeric table."""
import subprocess

import pyarrow as pa
import pytest

from arrow_go_amd import compute as ac

INTS = [pa.int8(), pa.uint8(), pa.int16(), pa.uint16(), pa.int32(), pa.uint32(), pa.int64(), pa.uint64()]
BINARY_LIKE = [pa.string(), pa.binary(), pa.large_string(), pa.large_binary()]
NEW_FUNCTIONS = ["cast_string", "cast_large_string", "cast_binary", "cast_large_binary", "cast_fixed_sized_binary"]


def test_registry_has_the_five_binary_cast_functions():
    for name in NEW_FUNCTIONS:
        assert ac.lib.ahc_has_function(name.encode()), name
    assert not ac.lib.ahc_has_function(b"cast_fixed_size_binary")   # the reference's spelling is "sized"


@pytest.mark.parametrize("name", ["cast_string", "cast_large_string"])
def test_string_targets_take_integers_boolean_and_binary_like(name):
    for frm in INTS + [pa.bool_()] + BINARY_LIKE:
        assert ac.dispatch_best(name, [frm]) == [frm], (name, frm)
    for frm in (pa.float64(), pa.float32()):                        # FormatFloat: out of scope
        with pytest.raises(ac.ErrNotImplemented, match="no kernel matching"):
            ac.dispatch_best(name, [frm])


@pytest.mark.parametrize("name", ["cast_binary", "cast_large_binary"])
def test_binary_targets_take_binary_like_only(name):
    for frm in BINARY_LIKE:
        assert ac.dispatch_best(name, [frm]) == [frm], (name, frm)
    for frm in (pa.int32(), pa.bool_(), pa.float64()):              # the reference registers no numeric → binary kernel
        with pytest.raises(ac.ErrNotImplemented, match="no kernel matching"):
            ac.dispatch_best(name, [frm])


def test_parse_kernels_sit_beside_the_numeric_tables():
    for to in INTS:
        for frm in BINARY_LIKE:
            assert ac.dispatch_best(f"cast_{to}", [frm]) == [frm], (to, frm)
    for frm in BINARY_LIKE:
        assert ac.dispatch_best("cast_boolean", [frm]) == [frm], frm
        for name in ("cast_float", "cast_double"):                  # ParseFloat: out of scope
            with pytest.raises(ac.ErrNotImplemented, match="no kernel matching"):
                ac.dispatch_best(name, [frm])
    # the reported tables are the numeric ones: nine other numeric types + Boolean
    assert ac.lib.ahc_function_num_kernels(b"cast_int32") == ac.lib.ahc_function_num_kernels(b"cast_double") == 10


def test_string_cast_entry_points_are_declared_and_exported():
    from arrow_go_amd import _native as N
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for sym in ("ah_parse_int", "ah_parse_bool", "ah_format_int_offsets", "ah_format_int_data", "ah_validate_utf8", "ah_fixed_binary_offsets"):
        assert sym in N.declared_symbols() and sym in exported, sym
