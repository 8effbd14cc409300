"""Array-level access to the C++ host layer (libarrowhip_compute.so), which mirrors
arrow-go's `compute.CallFunction` / function registry / `arrow/math` API on top of the HIP
kernels.  Arrays cross the boundary through the Arrow C Data Interface, exactly the route
arrow-go's own `arrow/cdata` package provides; pyarrow is only the producer/consumer of
those structs in the tests.

    s = Session(0)
    s.call_function("add", [pa.array([3, 2, 6]), pa.array([1, 0, 2])])   # → [4, 2, 8]
    s.call_function("filter", [values, mask], "null_selection_behavior=emit_null")

Errors mirror arrow-go's sentinel errors (arrow.ErrInvalid, ErrIndex, ErrNotImplemented,
"function '…' not found").  There is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import struct

from . import _native  # loads libarrowhip.so first (RTLD_GLOBAL)

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libarrowhip_compute.so")
if not os.path.exists(_LIB):
    raise ImportError(f"{_LIB} is missing — run __graft_entry__.build()")
lib = C.CDLL(_LIB)

_vp = C.c_void_p
lib.ahc_session_create.argtypes = [C.c_int, C.POINTER(_vp)]
lib.ahc_session_destroy.argtypes = [_vp]
lib.ahc_session_destroy.restype = None
lib.ahc_last_error.argtypes = [_vp]
lib.ahc_last_error.restype = C.c_char_p
lib.ahc_datum_release.argtypes = [_vp]
lib.ahc_datum_release.restype = None
lib.ahc_import.argtypes = [_vp, _vp, _vp, C.POINTER(_vp)]
lib.ahc_scalar.argtypes = [_vp, C.c_int, C.c_int, _vp, C.POINTER(_vp)]
lib.ahc_datum_info.argtypes = [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                               C.POINTER(C.c_int), _vp]
lib.ahc_call.argtypes = [_vp, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(_vp), C.POINTER(_vp)]
lib.ahc_export.argtypes = [_vp, _vp, _vp, _vp]
lib.ahc_import_host.argtypes = [_vp, _vp, _vp, C.POINTER(_vp)]
lib.ahc_datum_on_host.argtypes = [_vp]
lib.ahc_session_set_option.argtypes = [_vp, C.c_char_p, C.c_int64]
lib.ahc_math_sum.argtypes = [_vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
lib.ahc_has_function.argtypes = [C.c_char_p]
lib.ahc_function_num_kernels.argtypes = [C.c_char_p]
lib.ahc_registry_add_alias.argtypes = [_vp, C.c_char_p, C.c_char_p, C.c_int]
lib.ahc_import_device.argtypes = [_vp, _vp, _vp, C.POINTER(_vp)]
lib.ahc_export_device.argtypes = [_vp, _vp, _vp, _vp]
lib.ahc_datum_buffers.argtypes = [_vp, C.POINTER(_vp), C.POINTER(_vp)]
lib.ahc_chunked_from_arrays.argtypes = [_vp, C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(_vp)]
lib.ahc_datum_num_chunks.argtypes = [_vp]
lib.ahc_datum_chunk.argtypes = [_vp, _vp, C.c_int, C.POINTER(_vp)]
lib.ahc_record_from_arrays.argtypes = [_vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(_vp), C.POINTER(_vp)]
lib.ahc_record_num_columns.argtypes = [_vp]
lib.ahc_record_column.argtypes = [_vp, _vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(_vp)]
lib.ahc_ipc_open.argtypes = [_vp, _vp, C.c_int64, C.POINTER(_vp)]
lib.ahc_ipc_close.argtypes = [_vp]
lib.ahc_ipc_close.restype = None
lib.ahc_ipc_num_fields.argtypes = [_vp]
lib.ahc_ipc_field.argtypes = [_vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.ahc_ipc_next.argtypes = [_vp, C.POINTER(_vp), C.POINTER(C.c_int64)]
lib.ahc_datum_logical.argtypes = [_vp]
lib.ahc_datum_logical.restype = C.c_char_p
lib.ahc_scalar_bytes.argtypes = [_vp, C.c_char_p, C.c_int, C.c_char_p, C.c_int64, C.POINTER(_vp)]
lib.ahc_scalar_set_logical.argtypes = [_vp, _vp, C.c_char_p]
lib.ahc_ipc_bytes_uploaded.argtypes = [_vp]
lib.ahc_ipc_bytes_uploaded.restype = C.c_int64
lib.ahc_ipc_inspect.argtypes = [_vp, C.c_int64, C.c_char_p, C.c_int64]
lib.ahc_ipc_stats.argtypes = [_vp, C.POINTER(C.c_int64)]
lib.ahc_ipc_stats.restype = None
lib.ahc_ipc_writer_open.argtypes = [_vp, C.c_char_p, C.POINTER(_vp)]
lib.ahc_ipc_write_batch.argtypes = [_vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(_vp)]
lib.ahc_ipc_writer_finish.argtypes = [_vp, C.POINTER(_vp), C.POINTER(C.c_int64)]
lib.ahc_ipc_writer_stats.argtypes = [_vp, C.POINTER(C.c_int64)]
lib.ahc_ipc_writer_stats.restype = None
lib.ahc_ipc_writer_close.argtypes = [_vp]
lib.ahc_ipc_writer_close.restype = None
lib.ahc_substrait_inspect.argtypes = [_vp, C.c_int64, C.c_char_p, C.c_int64]
lib.ahc_dispatch_best.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int64]
lib.ahc_output_type.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int64]
lib.ahc_validate_options.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int64]
lib.ahc_like_compile.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_int64]
lib.ahc_like_compile.restype = C.c_int64
lib.ahc_expr_eval.argtypes = [_vp, C.c_char_p, C.c_int, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.c_int, C.POINTER(_vp), C.POINTER(C.c_int)]


class _ExprNode(C.Structure):   # ahc_expr_node of include/arrowhip_compute.h
    _fields_ = [("kind", C.c_int32), ("index", C.c_int32), ("name", C.c_char_p), ("options", C.c_char_p), ("nargs", C.c_int32), ("args", C.POINTER(C.c_int32))]


lib.ahc_expr_eval_tree.argtypes = [_vp, C.POINTER(_ExprNode), C.c_int, C.c_int, C.POINTER(_vp), C.POINTER(C.c_char_p), C.c_int, C.POINTER(_vp), C.c_int,
                                   C.POINTER(_vp), C.POINTER(C.c_int)]
lib.ahc_expr_eval_substrait.argtypes = [_vp, C.c_void_p, C.c_int64, C.c_int, C.POINTER(_vp), C.POINTER(C.c_char_p), C.c_int, C.POINTER(_vp), C.POINTER(C.c_int)]


# ---- Arrow C (Device) Data Interface structs (arrow/cdata/abi.h) ------------------------------------
class CArrowSchema(C.Structure):
    pass


CArrowSchema._fields_ = [("format", C.c_char_p), ("name", C.c_char_p), ("metadata", C.c_char_p), ("flags", C.c_int64),
                         ("n_children", C.c_int64), ("children", _vp), ("dictionary", _vp),
                         ("release", C.CFUNCTYPE(None, C.POINTER(CArrowSchema))), ("private_data", _vp)]


class CArrowArray(C.Structure):
    pass


CArrowArray._fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64),
                        ("n_children", C.c_int64), ("buffers", C.POINTER(_vp)), ("children", _vp), ("dictionary", _vp),
                        ("release", C.CFUNCTYPE(None, C.POINTER(CArrowArray))), ("private_data", _vp)]


class CArrowDeviceArray(C.Structure):
    _fields_ = [("array", CArrowArray), ("device_id", C.c_int64), ("device_type", C.c_int32), ("sync_event", _vp),
                ("reserved", C.c_int64 * 3)]


ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST = 1, 10, 11
_FORMATS = {"bool": b"b", "int8": b"c", "uint8": b"C", "int16": b"s", "uint16": b"S", "int32": b"i", "uint32": b"I", "int64": b"l",
            "uint64": b"L", "float": b"f", "double": b"g", "string": b"u", "binary": b"z", "large_string": b"U", "large_binary": b"Z"}


class DeviceArray:
    """An array datum that stays in HBM (an ahc_datum handle).  Pass it to call_function like a
    pyarrow array; `to_arrow()` downloads, `export_device()` hands the buffers to another ROCm consumer
    through the Arrow C Device Data Interface without a copy."""

    def __init__(self, session, handle):
        self.session, self.h = session, handle

    def buffers(self):
        v, d = _vp(), _vp()
        lib.ahc_datum_buffers(self.h, C.byref(v), C.byref(d))
        return v.value, d.value

    def to_arrow(self):
        return self.session._export(self.h)

    def on_host(self) -> bool:
        """True for a HOST-resident array: imported with Session.import_host / import_host_buffers, or the result of a call
        that streamed such arguments through the device (include/arrowhip_compute.h, "HOST-RESIDENT arguments")"""
        return bool(lib.ahc_datum_on_host(self.h))

    def export_device(self):
        """→ (CArrowDeviceArray, CArrowSchema); the caller owns them and must call array.release."""
        darr, sch = CArrowDeviceArray(), CArrowSchema()
        self.session._check(lib.ahc_export_device(self.session.h, self.h, C.addressof(darr), C.addressof(sch)))
        return darr, sch

    def release(self):
        if self.h:
            lib.ahc_datum_release(self.h)
            self.h = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class ArrowError(Exception):
    code = 0


class ErrInvalid(ArrowError):
    code = 1


class ErrIndex(ArrowError):
    code = 2


class ErrNotImplemented(ArrowError):
    code = 3


class ErrType(ArrowError):
    code = 4


class ErrKey(ArrowError):
    code = 5


class ErrHip(ArrowError):
    code = 6


_ERRS = {1: ErrInvalid, 2: ErrIndex, 3: ErrNotImplemented, 4: ErrType, 5: ErrKey, 6: ErrHip}

# arrow.Type ids
_TYPE_IDS = {"dictionary": 36, "string": 13, "binary": 14, "large_string": 34, "large_binary": 35, "bool": 1, "uint8": 2, "int8": 3, "uint16": 4, "int16": 5, "uint32": 6, "int32": 7, "uint64": 8, "int64": 9,
             "float": 11, "double": 12}
_PACK = {1: "<?", 2: "<B", 3: "<b", 4: "<H", 5: "<h", 6: "<I", 7: "<i", 8: "<Q", 9: "<q", 11: "<f", 12: "<d"}


_UNITS = {"s": "s", "m": "ms", "u": "us", "n": "ns"}


def _temporal_format(t):
    """pyarrow temporal type → its Arrow C Data format ("tsu:UTC", "tdD", "ttm", "tDn"), None for any other type"""
    import pyarrow as pa
    short = {v: k for k, v in _UNITS.items()}
    if pa.types.is_timestamp(t):
        return "ts%s:%s" % (short[t.unit], t.tz or "")
    if pa.types.is_duration(t):
        return "tD" + short[t.unit]
    if pa.types.is_date32(t):
        return "tdD"
    if pa.types.is_date64(t):
        return "tdm"
    if pa.types.is_time32(t) or pa.types.is_time64(t):
        return "tt" + short[t.unit]
    return None


def _bytes_format(t):
    """the Arrow C Data format of a byte-payload type (String, Binary, Large*, FixedSizeBinary, Decimal128 / 256), None otherwise"""
    import pyarrow as pa
    simple = {pa.string(): "u", pa.binary(): "z", pa.large_string(): "U", pa.large_binary(): "Z"}
    if t in simple:
        return simple[t]
    if pa.types.is_fixed_size_binary(t):
        return "w:%d" % t.byte_width
    if pa.types.is_decimal128(t):
        return "d:%d,%d" % (t.precision, t.scale)
    if pa.types.is_decimal256(t):
        return "d:%d,%d,256" % (t.precision, t.scale)
    return None


def _temporal_type(fmt):
    """the inverse: C Data format → pyarrow type"""
    import pyarrow as pa
    if fmt == "tdD":
        return pa.date32()
    if fmt == "tdm":
        return pa.date64()
    unit = _UNITS[fmt[2]]
    if fmt[1] == "t":
        return pa.time32(unit) if unit in ("s", "ms") else pa.time64(unit)
    if fmt[1] == "D":
        return pa.duration(unit)
    if fmt[1] == "s":
        return pa.timestamp(unit, tz=fmt[4:] or None)
    raise ErrNotImplemented(f"temporal format {fmt!r}")


def _as_bytes_ptr(buf):
    """(keep-alive object, address, length) of a bytes-like / pyarrow.Buffer without copying when possible"""
    mv = memoryview(buf)
    if mv.readonly:
        keep = (C.c_char * mv.nbytes).from_buffer_copy(mv) if not isinstance(buf, bytes) else buf
        addr = C.cast(C.c_char_p(keep), _vp).value if isinstance(keep, bytes) else C.addressof(keep)
        return keep, addr, mv.nbytes
    keep = (C.c_char * mv.nbytes).from_buffer(mv)
    return keep, C.addressof(keep), mv.nbytes



def dispatch_best(function: str, types):
    """fn.DispatchBest(types...) without executing (ahc_dispatch_best): pyarrow types in → the argument types of the chosen kernel
    as pyarrow types; raises the reference's error class (ErrNotImplemented "has no kernel matching input types", KeyError …)."""
    ids = {"bool": 1, "uint8": 2, "int8": 3, "uint16": 4, "int16": 5, "uint32": 6, "int32": 7, "uint64": 8, "int64": 9, "float": 11, "double": 12,
           "string": 13, "binary": 14, "large_string": 34, "large_binary": 35}
    back = {v: k for k, v in ids.items()}
    n = len(types)
    tin = (C.c_int * n)(*[ids[str(t)] for t in types])
    tout = (C.c_int * n)()
    err = C.create_string_buffer(1024)
    rc = lib.ahc_dispatch_best(function.encode(), n, tin, tout, err, len(err))
    if rc != 0:
        raise _ERRS.get(rc, ArrowError)(err.value.decode(errors="replace"))
    import pyarrow as pa
    named = {"float": pa.float32(), "double": pa.float64(), "bool": pa.bool_()}
    return [named.get(back[i], None) or getattr(pa, back[i])() for i in tout]

def output_type_id(function: str, type_ids) -> int:
    """The arrow.Type id of what the kernel DispatchBest chooses for these argument type ids returns (ahc_output_type; 0 where the
    call's options decide it), without a device; raises like dispatch_best."""
    n = len(type_ids)
    out = C.c_int()
    err = C.create_string_buffer(1024)
    rc = lib.ahc_output_type(function.encode(), n, (C.c_int * n)(*type_ids), C.byref(out), err, len(err))
    if rc != 0:
        raise _ERRS.get(rc, ArrowError)(err.value.decode(errors="replace"))
    return out.value


def validate_options(function: str, options: str) -> None:
    """What `function` answers to an options string before anything runs, without a device (ahc_validate_options): the string
    predicates check pattern_hex / ignore_case; raises the error class the call would raise."""
    err = C.create_string_buffer(1024)
    rc = lib.ahc_validate_options(function.encode(), options.encode(), err, len(err))
    if rc != 0:
        raise _ERRS.get(rc, ArrowError)(err.value.decode(errors="replace"))


def like_compile(pattern) -> bytes:
    """A SQL LIKE pattern (str or bytes; `%`, `_`, `\\` as in Arrow C++'s match_like) compiled on the host into the segment program
    Context.string_like takes (ahc_like_compile, host/like_program.h)."""
    pat = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
    out = C.create_string_buffer(3 + 4 * len(pat) + 8)
    n = lib.ahc_like_compile(C.c_char_p(pat), len(pat), out, len(out))
    if n < 0:
        raise ErrInvalid("like_compile: the program does not fit its buffer")
    return out.raw[:n]


def pattern_options(pattern, ignore_case: bool = False) -> str:
    """The options string of the string predicates: "pattern_hex=<the pattern's bytes in hex>" (a pattern may hold `;`, `=` or bytes
    that are no UTF-8), and "ignore_case=true" where asked — which the functions refuse with ErrNotImplemented."""
    pat = pattern.encode() if isinstance(pattern, str) else bytes(pattern)
    return "pattern_hex=" + pat.hex() + (";ignore_case=true" if ignore_case else "")


def slice_options(start: int, stop=None, step: int = 1) -> str:
    """The options string of utf8_slice_codeunits / binary_slice: "start=<int64>[;stop=<int64>][;step=<int64>]" — stop None: to the
    end of the row; a step other than 1 is written as it is, and the functions refuse it with ErrNotImplemented."""
    return "start=%d" % int(start) + ("" if stop is None else ";stop=%d" % int(stop)) + ("" if step == 1 else ";step=%d" % int(step))


def trim_options(characters) -> str:
    """The options string of ascii_trim / _ltrim / _rtrim and utf8_trim / _ltrim / _rtrim: "characters_hex=<the characters' bytes
    in hex>" (str or bytes; may be empty)."""
    chars = characters.encode() if isinstance(characters, str) else bytes(characters)
    return "characters_hex=" + chars.hex()


def inspect_substrait(buf) -> str:
    """What the Substrait reader understood of a serialized ExtendedExpression, without a device (ahc_substrait_inspect):
    "name:type,…|output_name=expression|…"; raises the reference's error class for a message the reader refuses as a whole."""
    keep, addr, n = _as_bytes_ptr(buf)
    out = C.create_string_buffer(1 << 16)
    rc = lib.ahc_substrait_inspect(addr, n, out, len(out))
    text = out.value.decode(errors="replace")
    if rc != 0:
        raise _ERRS.get(rc, ArrowError)(text)
    return text


def ipc_inspect(buf):
    """Walk an Arrow IPC stream on the host only (no GPU needed): → ([(name, type name, nullable)], [rows per batch]).
    Raises the same errors read_ipc would."""
    keep, addr, n = _as_bytes_ptr(buf)
    out = C.create_string_buffer(1 << 20)
    rc = lib.ahc_ipc_inspect(addr, n, out, len(out))
    text = out.value.decode()
    if rc != 0:
        raise _ERRS.get(rc, ArrowError)(text)
    names = {v: k for k, v in _TYPE_IDS.items()}
    fields, rows = text.split("|")
    fl = []
    for f in filter(None, fields.split(",")):
        nm, tid, nullable, logical = f.rsplit(":", 3)
        tname = str(_temporal_type(bytes.fromhex(logical).decode())) if logical and int(tid) != 36 else names[int(tid)]
        fl.append((bytes.fromhex(nm).decode("utf-8", "replace"), tname, nullable == "1"))
    return fl, [int(r) for r in rows.split(",") if r]


def has_function(name: str) -> bool:
    return bool(lib.ahc_has_function(name.encode()))


def function_num_kernels(name: str) -> int:
    return int(lib.ahc_function_num_kernels(name.encode()))


def num_functions() -> int:
    return int(lib.ahc_num_functions())


def select_k_options(k, sort_keys=None, order: str = "ascending", null_placement: str = "at_end") -> str:
    """The options string of select_k: "k=<k>" beside "sort_keys=<column>:<asc|desc>:<at_end|at_start>,…" (a record batch: most
    significant key first) or "order=…;null_placement=…" (one array).  Only what cannot be written into the string is refused
    here (k must be an integer >= 0); the keys are the library's to judge, as for sort_indices."""
    if isinstance(k, bool) or not isinstance(k, int) or k < 0:
        raise ValueError(f"select_k: k must be an integer >= 0, not {k!r}")
    if sort_keys is None:
        return f"k={k};order={order};null_placement={null_placement}"
    items = []
    for key in sort_keys:
        key = (key,) if isinstance(key, int) else tuple(key)
        col, ordr, npl = key[0], key[1] if len(key) > 1 else "asc", key[2] if len(key) > 2 else "at_end"
        items.append(f"{int(col)}:{ {'ascending': 'asc', 'descending': 'desc'}.get(ordr, ordr)}:{npl}")
    return "k=%d;sort_keys=%s" % (k, ",".join(items))


_ORDER_WORDS = {"asc": "asc", "ascending": "asc", "desc": "desc", "descending": "desc"}
_WINDOW_RANKS = ("row_number", "rank", "dense_rank")
_WINDOW_SCANS = ("cumulative_sum", "cumulative_min", "cumulative_max", "cumulative_count")


def _option_name(fn: str, name) -> str:
    """a column name that can stand in an options string"""
    if not isinstance(name, str) or not name:
        raise ValueError(f"{fn}: a column name must be a non-empty string, not {name!r}")
    if any(ch in name for ch in ",:;="):
        raise ValueError(f"{fn}: column name {name!r} cannot be written into an options string")
    return name


def window_options(partition_by=(), order_by=(), functions=()) -> str:
    """The options string of window: "partition_by=a,b;order_by=c:asc:at_end,d:desc:at_start;functions=row_number,cumulative_sum:v".
    partition_by: column names (or one name); order_by: names or (name, 'asc' | 'desc'[, 'at_end' | 'at_start']) tuples, most
    significant first; functions: 'row_number' | 'rank' | 'dense_rank' and (column, 'cumulative_sum' | 'cumulative_min' |
    'cumulative_max' | 'cumulative_count') pairs, as group_by takes its aggregates.  Refused here: what cannot be written into
    the string (names with ',', ':', ';' or '='), an unknown function, order or placement word, and an empty function list;
    what depends on the batch (unknown columns, types, duplicate output names, more than 7 order keys) is the library's to judge."""
    parts = [partition_by] if isinstance(partition_by, str) else list(partition_by or ())
    orders = [order_by] if isinstance(order_by, str) else list(order_by or ())
    funcs = [functions] if isinstance(functions, str) else list(functions or ())
    if not funcs:
        raise ValueError("window: no functions")
    okeys = []
    for key in orders:
        key = (key,) if isinstance(key, str) else tuple(key)
        if not 1 <= len(key) <= 3:
            raise ValueError(f"window: an order key is a name or (name, order[, null placement]), not {key!r}")
        ordr, npl = key[1] if len(key) > 1 else "asc", key[2] if len(key) > 2 else "at_end"
        if ordr not in _ORDER_WORDS:
            raise ValueError(f"window: order {ordr!r} of key {key[0]!r} is not asc or desc")
        if npl not in ("at_end", "at_start"):
            raise ValueError(f"window: null placement {npl!r} of key {key[0]!r} is not at_end or at_start")
        okeys.append("%s:%s:%s" % (_option_name("window", key[0]), _ORDER_WORDS[ordr], npl))
    items = []
    for f in funcs:
        if isinstance(f, str):
            if f not in _WINDOW_RANKS:
                raise ValueError(f"window: {f!r} is not a ranking function ({', '.join(_WINDOW_RANKS)}); a running aggregate is (column, function)")
            items.append(f)
            continue
        if len(f) != 2 or f[1] not in _WINDOW_SCANS:
            raise ValueError(f"window: a running aggregate is (column, function), function one of {', '.join(_WINDOW_SCANS)}, not {f!r}")
        items.append("%s:%s" % (f[1], _option_name("window", f[0])))
    return "partition_by=%s;order_by=%s;functions=%s" % (",".join(_option_name("window", p) for p in parts), ",".join(okeys), ",".join(items))


def rank_options(sort_keys=None, order: str = "ascending", null_placement: str = "at_end", tiebreaker: str = "min") -> str:
    """The options string of rank: "sort_keys=…" (a record batch: (column index, 'asc' | 'desc', 'at_end' | 'at_start'), most
    significant first, as select_k_options writes them) or "order=…;null_placement=…" (one array), then "tiebreaker=min|first|dense".
    tiebreaker 'max' is Arrow C++'s fourth choice and is not implemented: the library answers it with ErrNotImplemented."""
    if tiebreaker not in ("min", "first", "dense", "max"):
        raise ValueError(f"rank: tiebreaker {tiebreaker!r} is not min, first, dense or max")
    if sort_keys is None:
        return f"order={order};null_placement={null_placement};tiebreaker={tiebreaker}"
    items = []
    for key in sort_keys:
        key = (key,) if isinstance(key, int) else tuple(key)
        col, ordr, npl = key[0], key[1] if len(key) > 1 else "asc", key[2] if len(key) > 2 else "at_end"
        items.append(f"{int(col)}:{_ORDER_WORDS.get(ordr, ordr)}:{npl}")
    return "sort_keys=%s;tiebreaker=%s" % (",".join(items), tiebreaker)


class Session:
    """A device session: ah_ctx + ExecCtx with its own child registry."""

    def __init__(self, device_id: int = 0):
        h = _vp()
        rc = lib.ahc_session_create(device_id, C.byref(h))
        if rc != 0:
            raise ErrHip("ahc_session_create failed: is a GPU visible? (no CPU fallback)")
        self.h = h
        self.last_ipc_stats = dict(bytes_uploaded=0, device_buffers=0, host_buffers=0, device_fallbacks=0)   # of the latest read_ipc
        self.last_ipc_write_stats = dict(raw_bytes=0, body_bytes=0, buffers_compressed=0, buffers_raw=0)   # of the latest write_ipc
        self.device_id = device_id

    def close(self):
        if self.h:
            lib.ahc_session_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise _ERRS.get(rc, ArrowError)(lib.ahc_last_error(self.h).decode())

    # -- datum plumbing
    def _import(self, arr):
        import pyarrow as pa
        if isinstance(arr, pa.ChunkedArray):  # compute.ChunkedDatum: every chunk uploaded, chunk boundaries kept
            tname = str(arr.type)
            if pa.types.is_dictionary(arr.type):
                tid = 36  # arrow.DICTIONARY
            elif _temporal_format(arr.type):  # stored as integers of the type's width, labelled chunk by chunk
                tid = _TYPE_IDS["int32" if arr.type.bit_width == 32 else "int64"]
            elif tname in _TYPE_IDS:
                tid = _TYPE_IDS[tname]
            elif (pa.types.is_decimal(arr.type) or pa.types.is_fixed_size_binary(arr.type)) and arr.num_chunks:
                # parametric types: the id here, precision / scale / width from the chunks themselves
                tid = 23 if pa.types.is_decimal128(arr.type) else 24 if pa.types.is_decimal256(arr.type) else 15
            else:
                raise ErrNotImplemented(f"unsupported chunked type {tname}")
            parts = [self._import(c) for c in arr.chunks]
            try:
                d = _vp()
                handles = (_vp * max(len(parts), 1))(*parts)
                self._check(lib.ahc_chunked_from_arrays(self.h, tid, len(parts), handles, C.byref(d)))
                return d
            finally:
                for p in parts:
                    lib.ahc_datum_release(p)
        a = (C.c_uint8 * 80)()
        s = (C.c_uint8 * 72)()
        arr._export_to_c(C.addressof(a), C.addressof(s))
        d = _vp()
        self._check(lib.ahc_import(self.h, C.addressof(a), C.addressof(s), C.byref(d)))
        return d

    def _scalar(self, sc):
        import pyarrow as pa
        fmt = _bytes_format(sc.type)
        if fmt is not None:  # String / Binary / Large* / FixedSizeBinary / Decimal128 / Decimal256: ahc_scalar_bytes
            raw = b""
            if sc.is_valid:
                if pa.types.is_fixed_size_binary(sc.type) or pa.types.is_decimal(sc.type):
                    arr = pa.array([sc.as_py()], type=sc.type)
                    w = sc.type.byte_width
                    raw = arr.buffers()[1].to_pybytes()[arr.offset * w:(arr.offset + 1) * w]
                else:
                    v = sc.as_py()
                    raw = v.encode() if isinstance(v, str) else bytes(v)
            d = _vp()
            self._check(lib.ahc_scalar_bytes(self.h, fmt.encode(), int(sc.is_valid), raw, len(raw), C.byref(d)))
            return d
        logical = _temporal_format(sc.type)
        tid = _TYPE_IDS[("int32" if sc.type.bit_width == 32 else "int64") if logical else str(sc.type)]
        valid = sc.is_valid
        buf = (C.c_uint8 * 8)()
        if valid:
            raw = struct.pack(_PACK[tid], sc.value if logical else sc.as_py())
            C.memmove(buf, raw, len(raw))
        d = _vp()
        self._check(lib.ahc_scalar(self.h, tid, int(valid), buf, C.byref(d)))
        if logical:
            self._check(lib.ahc_scalar_set_logical(self.h, d, logical.encode()))
        return d

    def import_device(self, type_name: str, length: int, data_ptr, validity_ptr=None, null_count: int = 0, offset: int = 0,
                      sync_event=None, on_release=None, device_type: int = ARROW_DEVICE_ROCM, device_id=None, var_data_ptr=None,
                      n_buffers=None) -> "DeviceArray":
        """Consumer side of the Arrow C Device Data Interface (arrow/cdata/abi.h:66-128): wrap device
        buffers produced elsewhere WITHOUT copying them.  `on_release` is called when the library lets
        go of the producer's array (its release callback).  String / binary types: `data_ptr` is the offsets
        buffer, `var_data_ptr` the bytes (three buffers)."""
        fmt = _FORMATS[type_name]
        nb = n_buffers if n_buffers is not None else (3 if fmt in (b"u", b"z", b"U", b"Z") else 2)
        bufs = (_vp * 3)(validity_ptr, data_ptr, var_data_ptr)
        keep = {"bufs": bufs, "fmt": fmt}

        def _release_array(ptr):
            ptr.contents.release = C.cast(None, CArrowArray._fields_[8][1])
            if on_release:
                on_release()
            keep.clear()

        def _release_schema(ptr):
            ptr.contents.release = C.cast(None, CArrowSchema._fields_[7][1])

        rel_a = CArrowArray._fields_[8][1](_release_array)
        rel_s = CArrowSchema._fields_[7][1](_release_schema)
        keep["cb"] = (rel_a, rel_s)
        self._device_imports = getattr(self, "_device_imports", [])
        self._device_imports.append(keep)  # callbacks must outlive the C side's use of them
        darr = CArrowDeviceArray()
        darr.array.length, darr.array.null_count, darr.array.offset = length, null_count, offset
        darr.array.n_buffers, darr.array.n_children = nb, 0
        darr.array.buffers = C.cast(bufs, C.POINTER(_vp))
        darr.array.release = rel_a
        darr.device_id = self.device_id if device_id is None else device_id
        darr.device_type = device_type
        darr.sync_event = sync_event
        sch = CArrowSchema()
        sch.format, sch.name, sch.flags = fmt, b"", 2
        sch.release = rel_s
        d = _vp()
        self._check(lib.ahc_import_device(self.h, C.addressof(darr), C.addressof(sch), C.byref(d)))
        return DeviceArray(self, d)

    def set_option(self, name: str, value: int) -> None:
        """ExecCtx fields of this session: 'chunk_bytes' (ExecCtx.ChunkSize's role for host-resident arguments), 'host_threshold_bytes';
        for the read_ipc calls that follow: 'ipc_device_lz4' (1: LZ4_FRAME bodies of independent blocks are inflated in HBM, 0: on the
        host like every other compressed body), 'ipc_device_lz4_min_bytes' (smaller compressed bodies stay on the host);
        'select_k_route' (0: select_k chooses its route, 1: the radix route, 2: the sort with its final widening cut at k);
        'string_tile_bytes' (the LDS tile of the string searches: 0 the default, else 64 … 32768 — no result depends on it)."""
        self._check(lib.ahc_session_set_option(self.h, name.encode(), int(value)))

    def import_host(self, arr) -> "DeviceArray":
        """ahc_import_host of a pyarrow array: a flat fixed-width column of at least host_threshold_bytes stays in pyarrow's buffers
        (pageable memory: correct, but the copies do not overlap — use import_host_buffers with pinned memory for that)"""
        a = (C.c_uint8 * 80)()
        s = (C.c_uint8 * 72)()
        arr._export_to_c(C.addressof(a), C.addressof(s))
        d = _vp()
        self._check(lib.ahc_import_host(self.h, C.addressof(a), C.addressof(s), C.byref(d)))
        return DeviceArray(self, d)

    def import_host_buffers(self, type_name: str, length: int, data_ptr, validity_ptr=None, null_count: int = 0, offset: int = 0,
                            on_release=None) -> "DeviceArray":
        """ahc_import_host of raw host buffers (e.g. ah.Context.alloc_pinned memory): they stay where they are and must outlive the
        returned array; `on_release` is called when the library lets go of them"""
        fmt = _FORMATS[type_name]
        bufs = (_vp * 2)(validity_ptr, data_ptr)
        keep = {"bufs": bufs, "fmt": fmt}

        def _release_array(ptr):
            ptr.contents.release = C.cast(None, CArrowArray._fields_[8][1])
            if on_release:
                on_release()

        def _release_schema(ptr):
            ptr.contents.release = C.cast(None, CArrowSchema._fields_[7][1])

        rel_a = CArrowArray._fields_[8][1](_release_array)
        rel_s = CArrowSchema._fields_[7][1](_release_schema)
        keep["cb"] = (rel_a, rel_s)
        self._device_imports = getattr(self, "_device_imports", [])
        self._device_imports.append(keep)  # callbacks must outlive the C side's use of them
        arr = CArrowArray()
        arr.length, arr.null_count, arr.offset = length, null_count, offset
        arr.n_buffers, arr.n_children = 2, 0
        arr.buffers = C.cast(bufs, C.POINTER(_vp))
        arr.release = rel_a
        sch = CArrowSchema()
        sch.format, sch.name, sch.flags = fmt, b"", 2
        sch.release = rel_s
        d = _vp()
        self._check(lib.ahc_import_host(self.h, C.addressof(arr), C.addressof(sch), C.byref(d)))
        return DeviceArray(self, d)

    def _to_datum(self, x):
        import pyarrow as pa
        if isinstance(x, DeviceArray):
            return x.h
        if isinstance(x, (pa.Array, pa.ChunkedArray)):
            return self._import(x)
        if isinstance(x, pa.RecordBatch):  # compute.RecordDatum
            parts = [self._import(c) for c in x.columns]
            try:
                d = _vp()
                names = (C.c_char_p * max(len(parts), 1))(*[n.encode() for n in x.schema.names])
                handles = (_vp * max(len(parts), 1))(*parts)
                self._check(lib.ahc_record_from_arrays(self.h, len(parts), names, handles, C.byref(d)))
                return d
            finally:
                for p in parts:
                    lib.ahc_datum_release(p)
        if isinstance(x, pa.Scalar):
            return self._scalar(x)
        raise TypeError(f"unsupported argument {type(x)}: pass a pyarrow Array, ChunkedArray, RecordBatch or Scalar")

    def _export(self, d):
        import pyarrow as pa
        kind, tid, length, nulls, sv = C.c_int(), C.c_int(), C.c_int64(), C.c_int64(), C.c_int()
        val = (C.c_uint8 * 8)()
        lib.ahc_datum_info(d, C.byref(kind), C.byref(tid), C.byref(length), C.byref(nulls), C.byref(sv), val)
        if kind.value == 1:  # scalar
            name = {v: k for k, v in _TYPE_IDS.items()}[tid.value]
            typ = {"float": pa.float32(), "double": pa.float64(), "bool": pa.bool_()}.get(name) or getattr(pa, name)()
            logical = lib.ahc_datum_logical(d).decode()
            if not sv.value:
                return pa.scalar(None, type=_temporal_type(logical) if logical else typ)
            fmt = _PACK[tid.value]
            plain = pa.scalar(struct.unpack(fmt, bytes(val)[:struct.calcsize(fmt)])[0], type=typ)
            return plain.cast(_temporal_type(logical)) if logical else plain
        if kind.value == 4:  # record batch
            cols, names = [], []
            for i in range(lib.ahc_record_num_columns(d)):
                c, nm = _vp(), C.c_char_p()
                self._check(lib.ahc_record_column(self.h, d, i, C.byref(nm), C.byref(c)))
                names.append(nm.value.decode())
                try:
                    cols.append(self._export(c))
                finally:
                    lib.ahc_datum_release(c)
            return pa.RecordBatch.from_arrays(cols, names=names)
        if kind.value == 3:  # chunked
            parts = []
            for i in range(lib.ahc_datum_num_chunks(d)):
                c = _vp()
                self._check(lib.ahc_datum_chunk(self.h, d, i, C.byref(c)))
                try:
                    parts.append(self._export(c))
                finally:
                    lib.ahc_datum_release(c)
            if parts:
                return pa.chunked_array(parts)
            name = {v: k for k, v in _TYPE_IDS.items()}[tid.value]
            typ = {"float": pa.float32(), "double": pa.float64(), "bool": pa.bool_()}.get(name) or getattr(pa, name)()
            return pa.chunked_array([], type=typ)
        a = (C.c_uint8 * 80)()
        s = (C.c_uint8 * 72)()
        self._check(lib.ahc_export(self.h, d, C.addressof(a), C.addressof(s)))
        return pa.Array._import_from_c(C.addressof(a), C.addressof(s))

    # -- compute.CallFunction
    def call_function(self, name: str, args, options: str = "", value_set=None, keep_on_device: bool = False):
        """options: "key=value;…" (Go struct tags).  value_set: the SetOptions.ValueSet array of is_in.
        keep_on_device: return a DeviceArray (no download) — chain calls without leaving HBM."""
        datums = [self._to_datum(x) for x in args]
        borrowed_handles = [x.h.value for x in list(args) + ([value_set] if value_set is not None else []) if isinstance(x, DeviceArray)]
        if value_set is not None:
            vs = self._to_datum(value_set)
            datums.append(vs)  # released with the arguments
            options = (options + ";" if options else "") + "value_set=@%x" % vs.value
            nargs = len(datums) - 1
        else:
            nargs = len(datums)
        try:
            arr = (_vp * len(datums))(*datums)
            out = _vp()
            self._check(lib.ahc_call(self.h, name.encode(), options.encode(), nargs, arr, C.byref(out)))
            if keep_on_device:
                return DeviceArray(self, out)
            try:
                return self._export(out)
            finally:
                lib.ahc_datum_release(out)
        finally:
            for d in datums:
                if d.value not in borrowed_handles:  # DeviceArray arguments stay owned by their wrappers
                    lib.ahc_datum_release(d)

    def group_by(self, batch, keys, aggregates, keep_on_device: bool = False):
        """call_function("group_by", [batch], "keys=…;aggregates=…"): the groups of the record batch's key columns in first-seen order,
        the key columns first, then one column per aggregate named "<column>_<function>" (or "count_all").  aggregates: (column,
        function) pairs as pyarrow's Table.group_by(keys).aggregate(...) takes them — function one of sum, mean, min, max, count —
        and ([], "count_all"); variance and stddev (Float64, null where the group has no more than ddof valid values) also as (column,
        function, ddof), ddof an integer >= 0, default 0; count_distinct counts the distinct valid values of any column type a key may
        have, equal when their bytes are (-0.0 and +0.0 are two values).  The variance is taken about the Float64 mean of the column;
        for an Int64 or UInt64 column the `mean` aggregate stays the quotient of the wrapping 64-bit sum, as without a variance beside
        it, so where that sum wraps the two columns of a row do not belong together.  Above 4096 groups every pass of variance / stddev
        goes through device atomics: about 12 x the time of a Float64 `sum` at 2^16 groups.  Column names must not contain ',', ':',
        ';' or '='."""
        keys = [keys] if isinstance(keys, str) else list(keys)
        aggregates, items = list(aggregates), []
        for agg in aggregates:
            col, fn = agg[0], agg[1]
            if len(agg) == 3:
                if fn not in ("variance", "stddev"):
                    raise ValueError(f"group_by: ddof is an option of variance and stddev, not of {fn!r}")
                if isinstance(agg[2], bool) or not isinstance(agg[2], int) or agg[2] < 0:
                    raise ValueError(f"group_by: ddof must be an integer >= 0, not {agg[2]!r}")
                items.append(f"{fn}:{col}:{agg[2]}")
            elif len(agg) != 2:
                raise ValueError(f"group_by: an aggregate is (column, function) or (column, function, ddof), not {agg!r}")
            elif fn == "count_all":
                if col not in ([], (), None, ""):
                    raise ValueError(f"group_by: count_all takes no column, not {col!r}")
                items.append("count_all")
            else:
                items.append(f"{fn}:{col}")
        for name in keys + [str(agg[0]) for agg in aggregates if agg[1] != "count_all"]:
            if any(ch in name for ch in ",:;="):
                raise ValueError(f"group_by: column name {name!r} cannot be written into an options string")
        return self.call_function("group_by", [batch], "keys=%s;aggregates=%s" % (",".join(keys), ",".join(items)), keep_on_device=keep_on_device)

    def select_k(self, values, k, sort_keys=None, order: str = "ascending", null_placement: str = "at_end", keep_on_device: bool = False):
        """call_function("select_k", [values], "k=…;…"): the first min(k, rows) entries of sort_indices with the same keys — uint64
        row numbers, stable, NaNs next to the nulls — without sorting the column when the first key is an integer or float column
        (ORDER BY … LIMIT k).  values: an array, a chunked array or a record batch; sort_keys (a record batch): [(column index,
        'asc' | 'desc', 'at_end' | 'at_start'), …], most significant first; one array: order and null_placement.  The session
        option 'select_k_route' (0 auto, 1 radix, 2 sort) forces a route; the result does not depend on it."""
        return self.call_function("select_k", [values], select_k_options(k, sort_keys, order, null_placement), keep_on_device=keep_on_device)

    def window(self, batch, partition_by=(), order_by=(), functions=(), keep_on_device: bool = False):
        """call_function("window", [batch], window_options(...)): one value per INPUT row — the output has the batch's rows in the
        batch's order and one column per function: row_number, rank, dense_rank (UInt64, 1-based, never null) and
        "<column>_cumulative_sum" / "_min" / "_max" / "_count", the running aggregate over ROWS BETWEEN UNBOUNDED PRECEDING AND
        CURRENT ROW of the row's partition.  Partitions: rows equal on every partition_by column as group_by's keys are equal
        (bytes; a null is a value); no partition_by: one partition.  Order inside a partition: the stable sort order of order_by
        (as sort_indices orders; none: the input order).  Rows that tie on every order key are peers: they share a rank; with no
        order_by every row is its own peer group.  A running aggregate is null exactly where its input value is null and otherwise
        covers the valid values up to and including the row; cumulative_count is never null.  Sums: Int64 / UInt64 (wrapping) /
        Float64; min / max: the input type, NaNs ignored unless all values so far are NaN.  A pyarrow Table is taken when every
        column has one chunk.  Column names must not contain ',', ':', ';' or '='."""
        import pyarrow as pa
        if isinstance(batch, pa.Table):
            for name, col in zip(batch.schema.names, batch.columns):
                if col.num_chunks > 1:
                    raise ErrInvalid(f"window: column {name!r} is chunked ({col.num_chunks} chunks); combine_chunks() first")
            batch = pa.RecordBatch.from_arrays([c.chunk(0) if c.num_chunks else pa.array([], c.type) for c in batch.columns], names=batch.schema.names)
        return self.call_function("window", [batch], window_options(partition_by, order_by, functions), keep_on_device=keep_on_device)

    def rank(self, values, sort_keys=None, order: str = "ascending", null_placement: str = "at_end", tiebreaker: str = "min",
             keep_on_device: bool = False):
        """call_function("rank", [values], rank_options(...)): the 1-based UInt64 rank of every row in the sort order of
        sort_indices with the same keys — Arrow C++'s rank.  tiebreaker: 'min' rows that tie share the smallest of their positions
        (RANK()), 'first' ties numbered in input order (ROW_NUMBER()), 'dense' ranks without gaps (DENSE_RANK()).  Nulls tie with
        nulls, NaNs with NaNs, -0.0 with +0.0.  values: an array, a chunked array or a record batch with sort_keys."""
        return self.call_function("rank", [values], rank_options(sort_keys, order, null_placement, tiebreaker), keep_on_device=keep_on_device)

    # -- conditionals (Arrow C++'s semantics; every argument a pyarrow Array, ChunkedArray, Scalar or DeviceArray)
    def if_else(self, cond, left, right, keep_on_device: bool = False):
        """call_function("if_else", [cond, left, right]): row i is null where cond[i] is null, otherwise left[i] (cond true) or
        right[i] with that side's validity.  cond is Boolean; left and right have one type — numeric sides of different types are
        promoted by the rule `add` uses, every other pairing must match exactly.  Any argument may be a scalar; a scalar cond is
        decided on the host: one side is returned (a scalar side broadcast), an all-null column for a null cond.  Fixed-width sides:
        one streaming pass without a host synchronisation.  Under a null slot the payload is zero bytes, a null Boolean's data bit
        is 0, a null string has length 0."""
        return self.call_function("if_else", [cond, left, right], keep_on_device=keep_on_device)

    def coalesce(self, *values, keep_on_device: bool = False):
        """call_function("coalesce", values): per row the first valid value among the arguments, null if there is none.  One value
        type (numeric arguments are promoted as for if_else).  A right fold of if_else whose condition is the left argument's
        validity bitmap: k arguments cost k - 1 passes over the column, an argument without nulls ends the fold and is returned
        as it is."""
        return self.call_function("coalesce", list(values), keep_on_device=keep_on_device)

    def fill_null(self, values, fill_value, keep_on_device: bool = False):
        """call_function("fill_null", [values, fill_value]) = coalesce(values, fill_value): the nulls of `values` replaced by
        fill_value (a scalar or an array of the same length)."""
        return self.call_function("fill_null", [values, fill_value], keep_on_device=keep_on_device)

    def fill_null_forward(self, values, keep_on_device: bool = False):
        """call_function("fill_null_forward", [values]): a null row takes the nearest valid row before it and stays null when there
        is none (leading nulls).  Over a chunked array the carry crosses the chunk borders; the result is chunked like the input.
        A column without nulls is returned as it is.  At most 2^32 - 1 rows."""
        return self.call_function("fill_null_forward", [values], keep_on_device=keep_on_device)

    def fill_null_backward(self, values, keep_on_device: bool = False):
        """call_function("fill_null_backward", [values]): a null row takes the nearest valid row after it and stays null when there
        is none (trailing nulls); otherwise as fill_null_forward."""
        return self.call_function("fill_null_backward", [values], keep_on_device=keep_on_device)

    # -- string predicates (Arrow C++'s semantics; values a String / Binary / LargeString / LargeBinary Array, ChunkedArray or DeviceArray,
    # pattern str or bytes; the output's validity is the input's).  Session option 'string_tile_bytes' (0 = default) moves the tile
    # borders of the searches; no result depends on it.
    def match_substring(self, values, pattern, ignore_case: bool = False, keep_on_device: bool = False):
        """call_function("match_substring", [values], "pattern_hex=…"): Boolean, the pattern's bytes occur in the row; the empty pattern
        matches every row.  ignore_case=True is refused (ErrNotImplemented)."""
        return self.call_function("match_substring", [values], pattern_options(pattern, ignore_case), keep_on_device=keep_on_device)

    def starts_with(self, values, pattern, ignore_case: bool = False, keep_on_device: bool = False):
        """call_function("starts_with", [values], "pattern_hex=…"): Boolean, the row begins with the pattern's bytes."""
        return self.call_function("starts_with", [values], pattern_options(pattern, ignore_case), keep_on_device=keep_on_device)

    def ends_with(self, values, pattern, ignore_case: bool = False, keep_on_device: bool = False):
        """call_function("ends_with", [values], "pattern_hex=…"): Boolean, the row ends with the pattern's bytes."""
        return self.call_function("ends_with", [values], pattern_options(pattern, ignore_case), keep_on_device=keep_on_device)

    def find_substring(self, values, pattern, ignore_case: bool = False, keep_on_device: bool = False):
        """call_function("find_substring", [values], "pattern_hex=…"): Int32 (Int64 for the Large types), the byte index of the pattern's
        first occurrence in the row, -1 if there is none, 0 for the empty pattern."""
        return self.call_function("find_substring", [values], pattern_options(pattern, ignore_case), keep_on_device=keep_on_device)

    def match_like(self, values, pattern, ignore_case: bool = False, keep_on_device: bool = False):
        """call_function("match_like", [values], "pattern_hex=…"): Boolean, SQL LIKE over the whole row: `%` any run of bytes, `_` one
        character (a code point of a String / LargeString, a byte of a Binary / LargeBinary), `\\` makes the next pattern character
        literal, a trailing lone `\\` matches nothing."""
        return self.call_function("match_like", [values], pattern_options(pattern, ignore_case), keep_on_device=keep_on_device)

    def binary_length(self, values, keep_on_device: bool = False):
        """call_function("binary_length", [values]): Int32 (Int64 for the Large types), the bytes of the row; also FixedSizeBinary."""
        return self.call_function("binary_length", [values], keep_on_device=keep_on_device)

    def utf8_length(self, values, keep_on_device: bool = False):
        """call_function("utf8_length", [values]): Int32 / Int64, the code points of a String / LargeString row = its bytes that are not
        10xxxxxx continuation bytes (which is also what it counts on bytes that are no valid UTF-8)."""
        return self.call_function("utf8_length", [values], keep_on_device=keep_on_device)

    # -- string transforms (Arrow C++'s semantics; values a String / LargeString — binary_slice: Binary / LargeBinary — Array, ChunkedArray
    # or DeviceArray; the output has the input's type and validity, a null row has length 0).  Every result is one sub-range of the
    # row's bytes: ah_string_ranges + ah_string_gather.
    def ascii_upper(self, values, keep_on_device: bool = False):
        """call_function("ascii_upper", [values]): the bytes a-z become A-Z, every other byte (≥ 0x80 included) stays."""
        return self.call_function("ascii_upper", [values], keep_on_device=keep_on_device)

    def ascii_lower(self, values, keep_on_device: bool = False):
        """call_function("ascii_lower", [values]): the bytes A-Z become a-z, every other byte stays."""
        return self.call_function("ascii_lower", [values], keep_on_device=keep_on_device)

    def utf8_slice_codeunits(self, values, start: int, stop=None, step: int = 1, keep_on_device: bool = False):
        """call_function("utf8_slice_codeunits", [values], "start=…;stop=…"): Python's row[start:stop] over the row's code points (a
        byte that is not 10xxxxxx and the continuation bytes behind it; nothing is validated).  stop None: to the end of the row.
        step other than 1 is refused (ErrNotImplemented)."""
        return self.call_function("utf8_slice_codeunits", [values], slice_options(start, stop, step), keep_on_device=keep_on_device)

    def binary_slice(self, values, start: int, stop=None, step: int = 1, keep_on_device: bool = False):
        """call_function("binary_slice", [values], "start=…;stop=…"): Python's row[start:stop] over the bytes of a Binary / LargeBinary row."""
        return self.call_function("binary_slice", [values], slice_options(start, stop, step), keep_on_device=keep_on_device)

    def ascii_trim(self, values, characters, keep_on_device: bool = False):
        """call_function("ascii_trim", [values], "characters_hex=…"): the bytes of `characters` (a set of bytes) removed from both ends."""
        return self.call_function("ascii_trim", [values], trim_options(characters), keep_on_device=keep_on_device)

    def ascii_ltrim(self, values, characters, keep_on_device: bool = False):
        """… removed from the row's start."""
        return self.call_function("ascii_ltrim", [values], trim_options(characters), keep_on_device=keep_on_device)

    def ascii_rtrim(self, values, characters, keep_on_device: bool = False):
        """… removed from the row's end."""
        return self.call_function("ascii_rtrim", [values], trim_options(characters), keep_on_device=keep_on_device)

    def ascii_trim_whitespace(self, values, keep_on_device: bool = False):
        """call_function("ascii_trim_whitespace", [values]): the bytes 9-13 and 32 removed from both ends."""
        return self.call_function("ascii_trim_whitespace", [values], keep_on_device=keep_on_device)

    def ascii_ltrim_whitespace(self, values, keep_on_device: bool = False):
        """… removed from the row's start."""
        return self.call_function("ascii_ltrim_whitespace", [values], keep_on_device=keep_on_device)

    def ascii_rtrim_whitespace(self, values, keep_on_device: bool = False):
        """… removed from the row's end."""
        return self.call_function("ascii_rtrim_whitespace", [values], keep_on_device=keep_on_device)

    def utf8_trim(self, values, characters, keep_on_device: bool = False):
        """call_function("utf8_trim", [values], "characters_hex=…"): the code points of `characters` (valid UTF-8; a set of code
        points) removed from both ends."""
        return self.call_function("utf8_trim", [values], trim_options(characters), keep_on_device=keep_on_device)

    def utf8_ltrim(self, values, characters, keep_on_device: bool = False):
        """… removed from the row's start."""
        return self.call_function("utf8_ltrim", [values], trim_options(characters), keep_on_device=keep_on_device)

    def utf8_rtrim(self, values, characters, keep_on_device: bool = False):
        """… removed from the row's end."""
        return self.call_function("utf8_rtrim", [values], trim_options(characters), keep_on_device=keep_on_device)

    def hash_join(self, left, right, keys, right_keys=None, join_type: str = "inner", keep_on_device: bool = False):
        """call_function("hash_join", [left, right], "left_keys=…;right_keys=…;type=…"): the two record batches joined on their key
        columns (right_keys None: the same names as `keys`).  join_type: inner, left_outer, left_semi or left_anti.  Rows: the left rows
        in order, each with its right matches in order (left_outer: an unmatched left row once, nulls on the right); columns: every left
        column, then the right columns that are not keys (semi / anti: the left columns only).  Keys are equal when their bytes are; a
        null key matches nothing.  Column names must not contain ',', ';' or '='."""
        keys = [keys] if isinstance(keys, str) else list(keys)
        rkeys = None if right_keys is None else ([right_keys] if isinstance(right_keys, str) else list(right_keys))
        for name in keys + (rkeys or []) + [join_type]:
            if any(ch in name for ch in ",;="):
                raise ValueError(f"hash_join: {name!r} cannot be written into an options string")
        options = "left_keys=%s" % ",".join(keys)
        if rkeys is not None:
            options += ";right_keys=%s" % ",".join(rkeys)
        options += ";type=%s" % join_type
        return self.call_function("hash_join", [left, right], options, keep_on_device=keep_on_device)

    # -- ipc.NewReader / Reader.Next, with the record-batch bodies landing in HBM
    def read_ipc(self, buf):
        """Iterate the record batches of an Arrow IPC *stream* (bytes / pyarrow.Buffer / mmap): yields
        (field names, [DeviceArray per column], rows).  Each body goes to the device in one copy; the columns
        are slices of it.  `last_ipc_stats` follows the reader batch by batch: body bytes uploaded, and how many compressed buffers
        were inflated on the device, on the host, and on the host after the device decoder reported a status."""
        keep, addr, n = _as_bytes_ptr(buf)
        r = _vp()
        self._check(lib.ahc_ipc_open(self.h, addr, n, C.byref(r)))

        def note_stats():
            st = (C.c_int64 * 4)()
            lib.ahc_ipc_stats(r, st)
            self.last_ipc_stats = dict(zip(("bytes_uploaded", "device_buffers", "host_buffers", "device_fallbacks"), list(st)))

        try:
            nf = lib.ahc_ipc_num_fields(r)
            names = []
            for i in range(nf):
                nm = C.c_char_p()
                self._check(lib.ahc_ipc_field(r, i, C.byref(nm), None, None))
                names.append(nm.value.decode())
            while True:
                cols = (_vp * max(nf, 1))()
                rows = C.c_int64()
                self._check(lib.ahc_ipc_next(r, cols, C.byref(rows)))
                note_stats()
                if rows.value < 0:
                    return
                yield names, [DeviceArray(self, _vp(cols[i])) for i in range(nf)], rows.value
        finally:
            note_stats()
            lib.ahc_ipc_close(r)
            del keep

    # -- ipc.NewWriter / Writer.Write / Close, with the bodies compressed in HBM
    def write_ipc(self, names, batches, compression: str = "lz4") -> bytes:
        """The Arrow IPC *stream* of `batches` — an iterable of lists of DeviceArray, one per name, all of one length per batch —
        as bytes.  compression "lz4": every buffer is compressed on the device (LZ4 frames of independent 64 KiB blocks, which
        read_ipc inflates on the device) and only the compressed body comes down; "none": the plain body.  The first batch fixes
        the schema.  `last_ipc_write_stats`: plain bytes of all buffers, body bytes written, buffers written as frames, buffers
        written raw because their frame would not have been smaller."""
        if compression not in ("lz4", "none"):
            raise ValueError(f"write_ipc: compression must be 'lz4' or 'none', not {compression!r}")
        names = list(names)
        w = _vp()
        self._check(lib.ahc_ipc_writer_open(self.h, f"compression={compression}".encode(), C.byref(w)))

        def note_stats():
            st = (C.c_int64 * 4)()
            lib.ahc_ipc_writer_stats(w, st)
            self.last_ipc_write_stats = dict(zip(("raw_bytes", "body_bytes", "buffers_compressed", "buffers_raw"), list(st)))

        try:
            cnames = (C.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
            for batch in batches:
                batch = list(batch)
                if len(batch) != len(names):
                    raise ValueError(f"write_ipc: a batch of {len(batch)} columns for {len(names)} names")
                cols = (_vp * max(len(batch), 1))(*[c.h for c in batch])
                self._check(lib.ahc_ipc_write_batch(w, len(batch), cnames, cols))
                note_stats()
            p, n = _vp(), C.c_int64()
            self._check(lib.ahc_ipc_writer_finish(w, C.byref(p), C.byref(n)))
            return C.string_at(p.value, n.value) if n.value else b""
        finally:
            note_stats()
            lib.ahc_ipc_writer_close(w)

    # -- compute.Expression / exprs.ExecuteScalarExpression
    def eval_expression(self, text: str, columns, literals=(), fuse: bool = True, raw: bool = False):
        """Evaluate an expression tree over a batch.  `text` is prefix notation with `$i` for
        column i and `#k` for literal k, e.g. "greater(multiply_unchecked(add($0,$1),$2),#0)".
        fuse=True → one JIT-compiled kernel when the tree is fusible; fuse=False → one kernel per
        call node (the reference's executeScalarBatch).  Returns (result, fused)."""
        cols = [self._to_datum(c) for c in columns]
        lits = [self._to_datum(l) for l in literals]
        borrowed = [x.h.value for x in list(columns) + list(literals) if isinstance(x, DeviceArray)]   # stay owned by their wrappers
        try:
            ca = (_vp * max(len(cols), 1))(*cols)
            la = (_vp * max(len(lits), 1))(*lits)
            out = _vp()
            fused = C.c_int()
            self._check(lib.ahc_expr_eval(self.h, text.encode(), len(cols), ca, len(lits), la, int(fuse), C.byref(out), C.byref(fused)))
            try:
                return self._export(out), bool(fused.value)
            finally:
                lib.ahc_datum_release(out)
        finally:
            for d in cols + lits:
                if d.value not in borrowed:
                    lib.ahc_datum_release(d)

    def eval_expression_tree(self, tree, columns, names=None, fuse: bool = True):
        """The reference's own tree shape (compute.Expression: Literal | field reference | Call{name, args, options},
        arrow/compute/expression.go:52-78, 278-290) through ahc_expr_eval_tree.  tree: ("call", name, [subtrees], options text or None) |
        ("field", position or name) | ("lit", pyarrow scalar).  Returns (result, fused)."""
        nodes, lits, keep = [], [], []

        def walk(t):
            if t[0] == "lit":
                lits.append(t[1])
                nodes.append(_ExprNode(0, len(lits) - 1, None, None, 0, None))
            elif t[0] == "field":
                by_name = isinstance(t[1], str)
                nodes.append(_ExprNode(1, -1 if by_name else int(t[1]), t[1].encode() if by_name else None, None, 0, None))
            elif t[0] == "call":
                pos = [walk(a) for a in t[2]]
                arr = (C.c_int32 * max(len(pos), 1))(*pos)
                keep.append(arr)
                opts = t[3].encode() if len(t) > 3 and t[3] else None
                nodes.append(_ExprNode(2, 0, t[1].encode(), opts, len(pos), C.cast(arr, C.POINTER(C.c_int32))))
            else:
                raise ValueError(f"expression node kind {t[0]!r}")
            return len(nodes) - 1

        walk(tree)
        cols = [self._to_datum(c) for c in columns]
        ld = [self._to_datum(l) for l in lits]
        try:
            na = (_ExprNode * len(nodes))(*nodes)
            ca = (_vp * max(len(cols), 1))(*cols)
            la = (_vp * max(len(ld), 1))(*ld)
            nm = (C.c_char_p * max(len(cols), 1))(*[n.encode() for n in names]) if names is not None else None
            out, fused = _vp(), C.c_int()
            self._check(lib.ahc_expr_eval_tree(self.h, na, len(nodes), len(cols), ca, nm, len(ld), la, int(fuse), C.byref(out), C.byref(fused)))
            try:
                return self._export(out), bool(fused.value)
            finally:
                lib.ahc_datum_release(out)
        finally:
            for d in cols + ld:
                lib.ahc_datum_release(d)

    def eval_substrait(self, message: bytes, columns, names=None, fuse: bool = True):
        """exprs.ExecuteScalarSubstrait (arrow/compute/exprs/exec.go:465-488): `message` is a serialized substrait.ExtendedExpression
        with one referred expression; columns (pyarrow arrays / scalars / DeviceArrays) in base-schema order, or matched by `names`.
        Returns (result, fused)."""
        message = bytes(message)
        cols = [self._to_datum(c) for c in columns]
        try:
            ca = (_vp * max(len(cols), 1))(*cols)
            nm = (C.c_char_p * max(len(cols), 1))(*[n.encode() for n in names]) if names is not None else None
            buf = C.create_string_buffer(message, len(message))
            out, fused = _vp(), C.c_int()
            self._check(lib.ahc_expr_eval_substrait(self.h, C.cast(buf, C.c_void_p), len(message), len(cols), ca, nm, int(fuse), C.byref(out), C.byref(fused)))
            try:
                return self._export(out), bool(fused.value)
            finally:
                lib.ahc_datum_release(out)
        finally:
            for d in cols:
                lib.ahc_datum_release(d)

    # -- arrow/math
    def math_sum(self, arr):
        """math.Float64.Sum / Int64.Sum / Uint64.Sum of a pyarrow array or a DeviceArray"""
        resident = isinstance(arr, DeviceArray)
        d = arr.h if resident else self._import(arr)
        try:
            f, i, u = C.c_double(), C.c_int64(), C.c_uint64()
            self._check(lib.ahc_math_sum(self.h, d, C.byref(f), C.byref(i), C.byref(u)))
            if resident:
                kind, tid, length, nulls, sv = C.c_int(), C.c_int(), C.c_int64(), C.c_int64(), C.c_int()
                lib.ahc_datum_info(d, C.byref(kind), C.byref(tid), C.byref(length), C.byref(nulls), C.byref(sv), None)
                t = {v: k for k, v in _TYPE_IDS.items()}[tid.value]
            else:
                t = str(arr.type)
            return f.value if t == "double" else (i.value if t == "int64" else u.value)
        finally:
            if not resident:
                lib.ahc_datum_release(d)

    def add_alias(self, alias: str, existing: str, allow_overwrite: bool = False):
        self._check(lib.ahc_registry_add_alias(self.h, alias.encode(), existing.encode(), int(allow_overwrite)))
