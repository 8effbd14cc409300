"""Thin host-side handles over the C ABI: a context, device buffers, and one Python
method per leaf entry point taking DeviceBuffer / raw device pointers.

Harness-level plumbing used by tests/, bench.py and the array-level layer in
arrow_go_amd.compute; it adds no semantics of its own.  Everything executes in
libarrowhip.so on the GPU — there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _native as N
from ._native import lib, check


def _ptr(x) -> Optional[int]:
    """device pointer of a DeviceBuffer / DevicePtr / int / None"""
    if x is None:
        return None
    if isinstance(x, DeviceBuffer):
        return x.ptr
    return int(x)


class SortKey(C.Structure):
    """ah_sort_key (include/arrowhip.h)"""
    _fields_ = [("type", C.c_int), ("values", C.c_void_p), ("offsets", C.c_void_p), ("byte_width", C.c_int), ("valid", C.c_void_p),
                ("off", C.c_int64), ("descending", C.c_int), ("nulls_at_start", C.c_int)]


class GroupKey(C.Structure):
    """ah_group_key (include/arrowhip.h)"""
    _fields_ = [("offset_width", C.c_int), ("byte_width", C.c_int), ("bits", C.c_int), ("offsets", C.c_void_p), ("data", C.c_void_p),
                ("valid", C.c_void_p), ("off", C.c_int64)]


class DeviceBuffer:
    """A device allocation owned by a Context (ah_buf_alloc / ah_buf_free)."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(ctx.handle, lib.ah_buf_alloc(ctx.handle, self.nbytes, C.byref(p)))
        self.ptr = p.value or 0

    def at(self, byte_offset: int) -> int:
        return self.ptr + int(byte_offset)

    def upload(self, arr: np.ndarray, byte_offset: int = 0) -> "DeviceBuffer":
        a = np.ascontiguousarray(arr)
        assert byte_offset + a.nbytes <= max(self.nbytes, 1), "upload out of range"
        if a.nbytes:
            check(self.ctx.handle, lib.ah_upload_async(self.ctx.handle, self.ptr + byte_offset, a.ctypes.data, a.nbytes))
            self.ctx.sync()  # `a` may be a temporary
        return self

    def download(self, dtype, count: int, byte_offset: int = 0) -> np.ndarray:
        out = np.empty(int(count), dtype=dtype)
        if out.nbytes:
            check(self.ctx.handle, lib.ah_download_async(self.ctx.handle, out.ctypes.data, self.ptr + byte_offset, out.nbytes))
            self.ctx.sync()
        return out

    def memset(self, byte_value: int, nbytes: Optional[int] = None, byte_offset: int = 0) -> None:
        check(self.ctx.handle, lib.ah_memset_async(self.ctx.handle, self.ptr + byte_offset, byte_value,
                                                   self.nbytes if nbytes is None else nbytes))

    def free(self) -> None:
        if self.ptr:
            lib.ah_buf_free(self.ctx.handle, self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            if self.ptr and self.ctx.handle:
                self.free()
        except Exception:
            pass


class PinnedBuffer:
    """Pinned host memory from ah_host_alloc_pinned (what a Go memory.Allocator backed by go/arrowhip/allocator.go hands out),
    seen as a numpy array: the source / destination of overlapped transfers."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(ctx.handle, lib.ah_host_alloc_pinned(ctx.handle, max(self.nbytes, 1), C.byref(p)))
        self.ptr = p.value or 0
        self._raw = (C.c_uint8 * max(self.nbytes, 1)).from_address(self.ptr)

    def view(self, dtype, count: Optional[int] = None, byte_offset: int = 0) -> np.ndarray:
        dt = np.dtype(dtype)
        n = (self.nbytes - byte_offset) // dt.itemsize if count is None else int(count)
        return np.frombuffer(self._raw, dtype=dt, count=n, offset=byte_offset)

    def free(self) -> None:
        if self.ptr:
            self._raw = None
            lib.ah_host_free_pinned(self.ctx.handle, self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            if self.ptr and self.ctx.handle:
                self.free()
        except Exception:
            pass


def _hptr(x) -> Optional[int]:
    """host pointer of a numpy array / PinnedBuffer / int / None"""
    if x is None:
        return None
    if isinstance(x, PinnedBuffer):
        return x.ptr
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return x.ctypes.data
    return int(x)


class Ingest:
    """ah_ingest: chunked host → HBM pipeline with per-slot events (include/arrowhip.h, "overlapped host -> HBM ingest").
    Host arguments are numpy arrays (ideally views of a PinnedBuffer), PinnedBuffers or raw host addresses."""

    def __init__(self, ctx: "Context", chunk_bytes: int = 0, depth: int = 0):
        h = C.c_void_p()
        check(ctx.handle, lib.ah_ingest_create(ctx.handle, chunk_bytes, depth, C.byref(h)))
        self.ctx, self.handle = ctx, h

    def close(self) -> None:
        if self.handle:
            lib.ah_ingest_destroy(self.handle)
            self.handle = None

    def sum_float64(self, host, n: int) -> float:
        r = C.c_double()
        check(self.ctx.handle, lib.ah_ingest_sum_float64(self.handle, _hptr(host), n, C.byref(r)))
        return r.value

    def sum_int64(self, host, n: int) -> int:
        r = C.c_int64()
        check(self.ctx.handle, lib.ah_ingest_sum_int64(self.handle, _hptr(host), n, C.byref(r)))
        return r.value

    def arithmetic_binary(self, type_id: int, op: int, l_host, r_host, out_host, n: int) -> None:
        check(self.ctx.handle, lib.ah_ingest_arithmetic_binary(self.handle, type_id, op, _hptr(l_host), _hptr(r_host), _hptr(out_host), n))

    def filter_count(self, fdata_host, fvalid_host, foff: int, n: int, null_sel: int) -> int:
        r = C.c_int64()
        check(self.ctx.handle, lib.ah_ingest_filter_count(self.handle, _hptr(fdata_host), _hptr(fvalid_host), foff, n, null_sel, C.byref(r)))
        return r.value

    def filter_primitive(self, byte_width: int, values_host, vvalid_host, voff: int, n: int, n_out: int, out_values_host, out_valid_host) -> int:
        r = C.c_int64()
        check(self.ctx.handle, lib.ah_ingest_filter_primitive(self.handle, byte_width, _hptr(values_host), _hptr(vvalid_host), voff, n, n_out,
                                                              _hptr(out_values_host), _hptr(out_valid_host), C.byref(r)))
        return r.value


class Graph:
    """ah_graph: a captured sequence of calls, replayed with one submission (include/arrowhip.h, "hipGraph capture")"""

    def __init__(self, ctx: "Context", handle):
        self.ctx, self.handle = ctx, handle

    def launch(self) -> None:
        check(self.ctx.handle, lib.ah_graph_launch(self.ctx.handle, self.handle))

    def close(self) -> None:
        if self.handle:
            lib.ah_graph_destroy(self.handle)
            self.handle = None


class Comm:
    """ah_comm: this rank's RCCL communicator on an ah_ctx's compute stream (include/arrowhip.h, "multi-GPU exchange").
    Buffers are device pointers (ints, DeviceBuffers, or anything with .data_ptr())."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        st = lib.ah_comm_unique_id(C.addressof(buf))
        if st != N.AH_OK:
            raise N.ErrHip("ah_comm_unique_id failed: is librccl.so loadable?")
        return bytes(buf)

    def __init__(self, ctx: "Context", rank: int, world: int, unique_id: bytes):
        assert len(unique_id) == 128
        h = C.c_void_p()
        idb = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        check(ctx.handle, lib.ah_comm_init(ctx.handle, rank, world, C.addressof(idb), C.byref(h)))
        self.ctx, self.handle, self.rank, self.world = ctx, h, rank, world

    @classmethod
    def from_transport(cls, ctx: "Context", rank: int, world: int, transport) -> "Comm":
        """a communicator over a host-supplied transport (ah_comm_init_transport): `transport` has a `.struct` (AhTransport)
        whose callbacks stay alive with it — e.g. arrow_go_amd.distributed.GlooTransport"""
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(ctx.handle, lib.ah_comm_init_transport(ctx.handle, rank, world, C.byref(transport.struct), C.byref(h)))
        self.ctx, self.handle, self.rank, self.world, self._transport = ctx, h, rank, world, transport
        return self

    def close(self) -> None:
        if self.handle:
            lib.ah_comm_destroy(self.handle)
            self.handle = None

    # ---- configs C4 / C5 as single calls -------------------------------------------------------------------------------
    def cmp_filter_sum_i64(self, cmpop: int, x, valid, off: int, n_local: int, threshold: int):
        s, n = C.c_int64(), C.c_int64()
        check(self.ctx.handle, lib.ah_comm_cmp_filter_sum_i64(self.handle, cmpop, _ptr(x), _ptr(valid), off, n_local, threshold, C.byref(s), C.byref(n)))
        return s.value, n.value

    def cmp_filter_sum_f64(self, cmpop: int, x, valid, off: int, n_local: int, threshold: float):
        s, n = C.c_double(), C.c_int64()
        check(self.ctx.handle, lib.ah_comm_cmp_filter_sum_f64(self.handle, cmpop, _ptr(x), _ptr(valid), off, n_local, threshold, C.byref(s), C.byref(n)))
        return s.value, n.value

    def merge_groups(self, is_f64: bool, keys, sums, counts, first_rows, ngroups_local: int, row_offset: int, capacity: int,
                     out_keys, out_sums, out_counts, out_first_rows, null_group_local: int = -1, with_null_group: bool = False):
        """→ the global group count; with_null_group: → (count, position of the merged null group or -1).  null_group_local is what
        hash_sum reported for this rank's shard."""
        g = C.c_int64()
        ng = C.c_int32(-1)
        try:
            check(self.ctx.handle, lib.ah_comm_merge_groups(self.handle, int(is_f64), _ptr(keys), _ptr(sums), _ptr(counts), _ptr(first_rows),
                                                            ngroups_local, int(null_group_local), row_offset, capacity, _ptr(out_keys), _ptr(out_sums),
                                                            _ptr(out_counts), _ptr(out_first_rows), C.byref(g), C.byref(ng)))
        finally:
            self.last_ngroups = g.value      # set even when the capacity was too small
        return (g.value, ng.value) if with_null_group else g.value

    def allreduce_sum(self, type_id: int, send, recv, count: int) -> None:
        check(self.ctx.handle, lib.ah_comm_allreduce_sum(self.handle, type_id, _ptr(send), _ptr(recv), count))

    def allgather(self, send, recv, nbytes_per_rank: int) -> None:
        check(self.ctx.handle, lib.ah_comm_allgather(self.handle, _ptr(send), _ptr(recv), nbytes_per_rank))

    def alltoallv(self, send, send_bytes, send_offs, recv, recv_bytes, recv_offs) -> None:
        arr = lambda v: (C.c_int64 * self.world)(*[int(x) for x in v])
        check(self.ctx.handle, lib.ah_comm_alltoallv(self.handle, _ptr(send), arr(send_bytes), arr(send_offs), _ptr(recv), arr(recv_bytes), arr(recv_offs)))


class _SetChunk(C.Structure):  # ah_set_chunk (arrowhip.h)
    _fields_ = [("offset_width", C.c_int), ("offsets", C.c_void_p), ("data", C.c_void_p), ("valid", C.c_void_p), ("off", C.c_int64),
                ("n", C.c_int64)]


class _CmpOperand(C.Structure):  # ah_cmp_operand (arrowhip.h)
    _fields_ = [("offset_width", C.c_int), ("byte_width", C.c_int), ("offsets", C.c_void_p), ("data", C.c_void_p), ("off", C.c_int64),
                ("broadcast", C.c_int)]


class _CondSide(C.Structure):  # ah_cond_side (arrowhip.h)
    _fields_ = [("offset_width", C.c_int), ("byte_width", C.c_int), ("offsets", C.c_void_p), ("data", C.c_void_p), ("valid", C.c_void_p),
                ("off", C.c_int64), ("broadcast", C.c_int)]


def _cond_side(side) -> _CondSide:
    ow, bw, offsets, data, valid, off, broadcast = side
    return _CondSide(ow, bw, _ptr(offsets), _ptr(data), _ptr(valid), off, int(broadcast))


class Context:
    """ah_ctx: one GPU, a compute stream and a copy stream."""

    def __init__(self, device_id: int = 0, stream: Optional[int] = None):
        h = C.c_void_p()
        if stream is None:
            st = lib.ah_ctx_create(device_id, C.byref(h))
        else:
            st = lib.ah_ctx_create_on_stream(device_id, C.c_void_p(stream), C.byref(h))
        if st != N.AH_OK:
            raise N.ErrHip(f"ah_ctx_create(device={device_id}) failed with status {st}: is a GPU visible?")
        self.handle = h
        self.device_id = device_id

    # ---- lifecycle / memory ---------------------------------------------------------
    def close(self) -> None:
        if self.handle:
            lib.ah_ctx_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def sync(self) -> None:
        check(self.handle, lib.ah_sync(self.handle))

    def set_option(self, name: str, value: int) -> None:
        """measurement / test switch of this context (ah_ctx_set_option); never changes a result"""
        check(self.handle, lib.ah_ctx_set_option(self.handle, name.encode(), int(value)))

    # ---- hipGraph capture -------------------------------------------------------------------------------------------------
    def graph_begin(self) -> None:
        check(self.handle, lib.ah_graph_begin(self.handle))

    def graph_end(self) -> "Graph":
        h = C.c_void_p()
        check(self.handle, lib.ah_graph_end(self.handle, C.byref(h)))
        return Graph(self, h)

    def alloc_pinned(self, nbytes: int) -> PinnedBuffer:
        return PinnedBuffer(self, nbytes)

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def to_device(self, arr: np.ndarray, pad: int = 0) -> DeviceBuffer:
        a = np.ascontiguousarray(arr)
        return DeviceBuffer(self, a.nbytes + pad).upload(a)

    def timer_start(self) -> None:
        check(self.handle, lib.ah_timer_start(self.handle))

    def timer_stop(self) -> float:
        ms = C.c_float()
        check(self.handle, lib.ah_timer_stop(self.handle, C.byref(ms)))
        return ms.value

    def event_record(self, slot: int) -> None:
        check(self.handle, lib.ah_event_record(self.handle, slot))

    def event_elapsed_ms(self, slot_a: int, slot_b: int) -> float:
        ms = C.c_float()
        check(self.handle, lib.ah_event_elapsed_ms(self.handle, slot_a, slot_b, C.byref(ms)))
        return ms.value

    # ---- arrow/math Sum -----------------------------------------------------------------
    def sum_float64(self, buf, n: int) -> float:
        r = C.c_double()
        check(self.handle, lib.ah_sum_float64(self.handle, _ptr(buf), n, C.byref(r)))
        return r.value

    def sum_int64(self, buf, n: int) -> int:
        r = C.c_int64()
        check(self.handle, lib.ah_sum_int64(self.handle, _ptr(buf), n, C.byref(r)))
        return r.value

    def sum_uint64(self, buf, n: int) -> int:
        r = C.c_uint64()
        check(self.handle, lib.ah_sum_uint64(self.handle, _ptr(buf), n, C.byref(r)))
        return r.value

    def sum_float64_dev(self, buf, n: int, res_dev) -> None:
        check(self.handle, lib.ah_sum_float64_dev(self.handle, _ptr(buf), n, _ptr(res_dev)))

    def sum_int64_dev(self, buf, n: int, res_dev) -> None:
        check(self.handle, lib.ah_sum_int64_dev(self.handle, _ptr(buf), n, _ptr(res_dev)))

    # ---- arithmetic ---------------------------------------------------------------------
    def arithmetic(self, type_id: int, op: int, shape: int, l, r, out, n: int) -> None:
        """l / r: device pointer, or (for the scalar side of AS / SA) a numpy scalar array."""
        if shape == N.SHAPE_AA:
            st = lib.ah_arithmetic_binary(self.handle, type_id, op, _ptr(l), _ptr(r), _ptr(out), n)
        elif shape == N.SHAPE_AS:
            s = np.ascontiguousarray(r)
            st = lib.ah_arithmetic_arr_scalar(self.handle, type_id, op, _ptr(l), s.ctypes.data, _ptr(out), n)
        else:
            s = np.ascontiguousarray(l)
            st = lib.ah_arithmetic_scalar_arr(self.handle, type_id, op, s.ctypes.data, _ptr(r), _ptr(out), n)
        check(self.handle, st)

    def arithmetic_unary(self, type_id: int, op: int, inp, out, n: int) -> None:
        check(self.handle, lib.ah_arithmetic_unary(self.handle, type_id, op, _ptr(inp), _ptr(out), n))

    def arithmetic_checked(self, type_id: int, op: int, shape: int, l, lvalid, loff, r, rvalid, roff, scalar_valid,
                           out, n: int) -> None:
        keep = []

        def side(x, is_scalar):
            if is_scalar:
                s = np.ascontiguousarray(x)
                keep.append(s)
                return s.ctypes.data
            return _ptr(x)

        st = lib.ah_arithmetic_checked(self.handle, type_id, op, shape, side(l, shape == N.SHAPE_SA), _ptr(lvalid), loff,
                                       side(r, shape == N.SHAPE_AS), _ptr(rvalid), roff, int(scalar_valid), _ptr(out), n)
        check(self.handle, st)

    def arithmetic_ext(self, type_id: int, op: int, shape: int, l, lvalid, loff, r, rvalid, roff, scalar_valid, out, n: int) -> None:
        """divide / abs / negate (checked) / bit-wise / shifts / sqrt — see ah_arithmetic_ext; unary ops: r = None"""
        keep = []

        def side(x, is_scalar):
            if x is None:
                return None
            if is_scalar:
                s = np.ascontiguousarray(x)
                keep.append(s)
                return s.ctypes.data
            return _ptr(x)

        st = lib.ah_arithmetic_ext(self.handle, type_id, op, shape, side(l, shape == N.SHAPE_SA), _ptr(lvalid), loff,
                                   side(r, shape == N.SHAPE_AS), _ptr(rvalid), roff, int(scalar_valid), _ptr(out), n)
        check(self.handle, st)

    def round(self, type_id: int, values, valid, off: int, n: int, ndigits: int, mode: int, multiple, pow10: float, out) -> None:
        """round (multiple=None; pow10 = math.Pow10(|ndigits|)) / round_to_multiple (multiple: numpy scalar array of the type)"""
        m = None if multiple is None else np.ascontiguousarray(multiple)
        check(self.handle, lib.ah_round(self.handle, type_id, _ptr(values), _ptr(valid), off, n, ndigits, mode,
                                        None if m is None else m.ctypes.data, float(pow10), _ptr(out)))

    # ---- compare ------------------------------------------------------------------------
    def comparison(self, cmpop: int, shape: int, type_id: int, l, r, out_bits, n: int, out_bit_offset: int = 0) -> None:
        keep = []

        def side(x, is_scalar):
            if is_scalar:
                s = np.ascontiguousarray(x)
                keep.append(s)
                return s.ctypes.data
            return _ptr(x)

        st = lib.ah_comparison(self.handle, cmpop, shape, type_id, side(l, shape == N.SHAPE_SA),
                               side(r, shape == N.SHAPE_AS), _ptr(out_bits), n, out_bit_offset)
        check(self.handle, st)

    # ---- bitmaps ------------------------------------------------------------------------
    def bitmap_op(self, op: int, l, loff: int, r, roff: int, out, ooff: int, nbits: int) -> None:
        check(self.handle, lib.ah_bitmap_op(self.handle, op, _ptr(l), loff, _ptr(r), roff, _ptr(out), ooff, nbits))

    def count_set_bits(self, bits, off: int, nbits: int) -> int:
        r = C.c_int64()
        check(self.handle, lib.ah_count_set_bits(self.handle, _ptr(bits), off, nbits, C.byref(r)))
        return r.value

    def copy_bitmap(self, src, soff: int, nbits: int, dst, doff: int, invert: bool = False) -> None:
        check(self.handle, lib.ah_copy_bitmap(self.handle, _ptr(src), soff, nbits, _ptr(dst), doff, int(invert)))

    def set_bits_to(self, bits, off: int, nbits: int, value: bool) -> None:
        check(self.handle, lib.ah_set_bits_to(self.handle, _ptr(bits), off, nbits, int(value)))

    def kleene(self, op: int, lvalid, ldata, loff: int, rvalid, rdata, roff: int, ovalid, odata, ooff: int, nbits: int) -> None:
        check(self.handle, lib.ah_kleene(self.handle, op, _ptr(lvalid), _ptr(ldata), loff, _ptr(rvalid), _ptr(rdata), roff,
                                         _ptr(ovalid), _ptr(odata), ooff, nbits))

    # ---- selection ----------------------------------------------------------------------
    def filter_count(self, fdata, fvalid, foff: int, n: int, null_sel: int) -> int:
        r = C.c_int64()
        check(self.handle, lib.ah_filter_count(self.handle, _ptr(fdata), _ptr(fvalid), foff, n, null_sel, C.byref(r)))
        return r.value

    def filter_primitive(self, byte_width: int, values, vvalid, voff: int, fdata, fvalid, foff: int, n: int, null_sel: int,
                         n_out: int, out_values, out_valid, want_null_count: bool = True) -> int:
        r = C.c_int64()
        check(self.handle, lib.ah_filter_primitive(self.handle, byte_width, _ptr(values), _ptr(vvalid), voff, _ptr(fdata),
                                                   _ptr(fvalid), foff, n, null_sel, n_out, _ptr(out_values), _ptr(out_valid),
                                                   C.byref(r) if want_null_count else None))
        return r.value

    def filter_primitive_dev(self, byte_width: int, values, vvalid, voff: int, fdata, fvalid, foff: int, n: int, null_sel: int,
                             out_values, out_valid, status_dev) -> None:
        """No count call, no host round trip: outputs sized for n rows, {selected, null count} left in `status_dev` (16 bytes)."""
        check(self.handle, lib.ah_filter_primitive_dev(self.handle, byte_width, _ptr(values), _ptr(vvalid), voff, _ptr(fdata),
                                                       _ptr(fvalid), foff, n, null_sel, _ptr(out_values), _ptr(out_valid), _ptr(status_dev)))

    def filter_primitive_once(self, byte_width: int, values, vvalid, voff: int, fdata, fvalid, foff: int, n: int, null_sel: int,
                              out_values, out_valid):
        """PrimitiveFilter in ONE call: outputs sized for n rows (the worst case), → (rows selected, output null count)."""
        k, nulls = C.c_int64(), C.c_int64()
        check(self.handle, lib.ah_filter_primitive_once(self.handle, byte_width, _ptr(values), _ptr(vvalid), voff, _ptr(fdata),
                                                        _ptr(fvalid), foff, n, null_sel, _ptr(out_values), _ptr(out_valid),
                                                        C.byref(k), C.byref(nulls)))
        return k.value, nulls.value

    def take_primitive_dev(self, byte_width: int, values, vvalid, voff: int, nvalues: int, idx_byte_width: int, idx_signed: bool,
                           idx, ivalid, ioff: int, nidx: int, out_values, out_valid, status_dev) -> None:
        """No host round trip: {position of the first out-of-range index or 2^64 − 1, null count} left in `status_dev` (16 bytes)."""
        check(self.handle, lib.ah_take_primitive_dev(self.handle, byte_width, _ptr(values), _ptr(vvalid), voff, nvalues,
                                                     idx_byte_width, int(idx_signed), _ptr(idx), _ptr(ivalid), ioff, nidx,
                                                     _ptr(out_values), _ptr(out_valid), _ptr(status_dev)))

    def filter_to_indices(self, fdata, fvalid, foff: int, n: int, null_sel: int, n_out: int, out_idx, out_valid) -> int:
        r = C.c_int64()
        check(self.handle, lib.ah_filter_to_indices(self.handle, _ptr(fdata), _ptr(fvalid), foff, n, null_sel, n_out,
                                                    _ptr(out_idx), _ptr(out_valid), C.byref(r)))
        return r.value

    def take_primitive(self, byte_width: int, values, vvalid, voff: int, nvalues: int, idx_byte_width: int, idx_signed: bool,
                       idx, ivalid, ioff: int, nidx: int, bounds_check: bool, out_values, out_valid) -> int:
        r = C.c_int64()
        bad = C.c_int64()
        check(self.handle, lib.ah_take_primitive(self.handle, byte_width, _ptr(values), _ptr(vvalid), voff, nvalues,
                                                 idx_byte_width, int(idx_signed), _ptr(idx), _ptr(ivalid), ioff, nidx,
                                                 int(bounds_check), _ptr(out_values), _ptr(out_valid), C.byref(r), C.byref(bad)))
        return r.value

    # ---- cumulative_sum -----------------------------------------------------------------
    def cumulative_sum(self, type_id: int, values, valid, off: int, n: int, start: Optional[bytes], skip_nulls: bool, checked: bool,
                       out_values, out_valid) -> int:
        """start: little-endian payload of one element of the type, or None (= 0).  Returns the output null count."""
        nulls = C.c_int64()
        sbuf = None
        if start is not None:
            sbuf = (C.c_uint8 * 8)()
            C.memmove(sbuf, start, len(start))
        check(self.handle, lib.ah_cumulative_sum(self.handle, type_id, _ptr(values), _ptr(valid), off, n,
                                                 C.addressof(sbuf) if sbuf is not None else None, int(skip_nulls), int(checked),
                                                 _ptr(out_values), _ptr(out_valid),
                                                 C.byref(nulls) if out_valid is not None else None))  # no validity → no sync
        return nulls.value

    # ---- cast ---------------------------------------------------------------------------
    def cast_numeric(self, in_type: int, out_type: int, values, valid, off: int, n: int, allow_int_overflow: bool,
                     allow_float_truncate: bool, out_values) -> None:
        check(self.handle, lib.ah_cast_numeric(self.handle, in_type, out_type, _ptr(values), _ptr(valid), off, n,
                                               int(allow_int_overflow), int(allow_float_truncate), _ptr(out_values)))

    def cast_decimal_rescale(self, in_width: int, out_width: int, scale_delta: int, out_precision: int, allow_truncate: bool, values, valid,
                             off: int, n: int, out_values) -> None:
        """CastDecimalToDecimal (numeric_cast.go:377-429); widths in bytes (16 | 32), scale_delta = out scale − in scale"""
        check(self.handle, lib.ah_cast_decimal_rescale(self.handle, in_width, out_width, scale_delta, out_precision, int(allow_truncate),
                                                       _ptr(values), _ptr(valid), off, n, _ptr(out_values)))

    def cast_int_to_decimal(self, in_type: int, out_width: int, scale: int, values, valid, off: int, n: int, out_values) -> None:
        """CastIntegerToDecimal (numeric_cast.go:173-239): value · 10^scale"""
        check(self.handle, lib.ah_cast_int_to_decimal(self.handle, in_type, out_width, scale, _ptr(values), _ptr(valid), off, n, _ptr(out_values)))

    def cast_decimal_to_int(self, in_width: int, in_scale: int, out_type: int, allow_truncate: bool, allow_overflow: bool, values, valid,
                            off: int, n: int, out_values) -> None:
        """CastDecimal128ToInteger / CastDecimal256ToInteger (numeric_cast.go:79-171)"""
        check(self.handle, lib.ah_cast_decimal_to_int(self.handle, in_width, in_scale, out_type, int(allow_truncate), int(allow_overflow),
                                                      _ptr(values), _ptr(valid), off, n, _ptr(out_values)))

    def shift_time(self, in_bits: int, out_bits: int, op: int, factor: int, checked: bool, values, valid, off: int, n: int, out_values) -> None:
        """ShiftTime (cast_temporal.go:35-104); op 0 multiply, 1 divide.  A failed check raises ErrInvalid carrying .bad_value"""
        bad = C.c_int64(0)
        try:
            check(self.handle, lib.ah_shift_time(self.handle, in_bits, out_bits, op, factor, int(checked), _ptr(values), _ptr(valid), off, n,
                                                        _ptr(out_values), C.byref(bad)))
        except N.ErrInvalid as e:
            e.bad_value = bad.value
            raise

    # ---- string casts (ah_cast_string.hip) -------------------------------------------------
    def parse_int(self, offset_width: int, offsets, data, valid, off: int, n: int, out_type: int, out_values) -> None:
        """strconv.ParseInt / ParseUint(s, 0, bits) per valid row (numeric_cast.go:742-781).  The LAST offending valid row raises
        ErrInvalid carrying .bad_row (relative to off) and .bad_kind (1 syntax, 2 range)"""
        bad, kind = C.c_int64(-1), C.c_int(0)
        try:
            check(self.handle, lib.ah_parse_int(self.handle, offset_width, _ptr(offsets), _ptr(data), _ptr(valid), off, n, out_type, _ptr(out_values),
                                                C.byref(bad), C.byref(kind)))
        except N.ErrInvalid as e:
            e.bad_row, e.bad_kind = bad.value, kind.value
            raise

    def parse_bool(self, offset_width: int, offsets, data, valid, off: int, n: int, out_bits) -> None:
        """strconv.ParseBool per valid row into a bitmap from bit 0 (boolean_cast.go:77-95); errors as parse_int"""
        bad = C.c_int64(-1)
        try:
            check(self.handle, lib.ah_parse_bool(self.handle, offset_width, _ptr(offsets), _ptr(data), _ptr(valid), off, n, _ptr(out_bits), C.byref(bad)))
        except N.ErrInvalid as e:
            e.bad_row, e.bad_kind = bad.value, 1
            raise

    def format_int_offsets(self, in_type: int, values, valid, off: int, n: int, offset_width: int, out_offsets) -> int:
        """offsets of the integer / boolean (in_type 1: `values` is the data bitmap) → string cast; returns the byte total"""
        total = C.c_int64(0)
        check(self.handle, lib.ah_format_int_offsets(self.handle, in_type, _ptr(values), _ptr(valid), off, n, offset_width, _ptr(out_offsets), C.byref(total)))
        return total.value

    def format_int_data(self, in_type: int, values, valid, off: int, n: int, offset_width: int, out_offsets, out_data) -> None:
        """the characters of strconv.FormatInt / FormatUint / FormatBool, given format_int_offsets' offsets of the same column"""
        check(self.handle, lib.ah_format_int_data(self.handle, in_type, _ptr(values), _ptr(valid), off, n, offset_width, _ptr(out_offsets), _ptr(out_data)))

    def validate_utf8(self, offset_width: int, offsets, data, byte_width: int, valid, off: int, n: int) -> None:
        """utf8.Valid of every valid row (string_casts.go:39-87); offset_width 0: fixed-size rows.  The FIRST offending valid row raises
        ErrInvalid carrying .bad_row"""
        bad = C.c_int64(-1)
        try:
            check(self.handle, lib.ah_validate_utf8(self.handle, offset_width, _ptr(offsets), _ptr(data), byte_width, _ptr(valid), off, n, C.byref(bad)))
        except N.ErrInvalid as e:
            e.bad_row = bad.value
            raise

    def fixed_binary_offsets(self, offset_width: int, byte_width: int, off: int, n: int, out_offsets) -> None:
        """CastFsbToBinary's offsets (string_casts.go:154-193): (off + i) · byte_width, i = 0 … n"""
        check(self.handle, lib.ah_fixed_binary_offsets(self.handle, offset_width, byte_width, off, n, _ptr(out_offsets)))

    def cast_bool_to_numeric(self, out_type: int, bits, off: int, n: int, out_values) -> None:
        check(self.handle, lib.ah_cast_bool_to_numeric(self.handle, out_type, _ptr(bits), off, n, _ptr(out_values)))

    # ---- set lookup ---------------------------------------------------------------------
    def is_in(self, byte_width: int, values, valid, off: int, n: int, set_values, set_valid, set_off: int, set_n: int,
              null_behavior: int, out_data, out_valid, out_bit_offset: int = 0) -> None:
        check(self.handle, lib.ah_is_in(self.handle, byte_width, _ptr(values), _ptr(valid), off, n, _ptr(set_values), _ptr(set_valid),
                                        set_off, set_n, null_behavior, _ptr(out_data), _ptr(out_valid), out_bit_offset))

    @staticmethod
    def _set_pieces(pieces):
        """[(offset_width, offsets, data, valid, off, n), …] → an ah_set_chunk table (offset_width 0: fixed-width piece)"""
        tbl = (_SetChunk * max(len(pieces), 1))()
        for i, (ow, offs, data, valid, off, n) in enumerate(pieces):
            tbl[i] = _SetChunk(ow, _ptr(offs), _ptr(data), _ptr(valid), off, n)
        return tbl

    def is_in_binary(self, offset_width: int, offsets, data, valid, off: int, n: int, set_pieces, null_behavior: int, out_data, out_valid,
                     out_bit_offset: int = 0) -> None:
        tbl = self._set_pieces(set_pieces)
        check(self.handle, lib.ah_is_in_binary(self.handle, offset_width, _ptr(offsets), _ptr(data), _ptr(valid), off, n, len(set_pieces), tbl,
                                               null_behavior, _ptr(out_data), _ptr(out_valid), out_bit_offset))

    def is_in_fixed(self, byte_width: int, data, valid, off: int, n: int, set_pieces, null_behavior: int, out_data, out_valid,
                    out_bit_offset: int = 0) -> None:
        tbl = self._set_pieces(set_pieces)
        check(self.handle, lib.ah_is_in_fixed(self.handle, byte_width, _ptr(data), _ptr(valid), off, n, len(set_pieces), tbl, null_behavior,
                                              _ptr(out_data), _ptr(out_valid), out_bit_offset))

    def is_in_dict_gather(self, index_width: int, indices, valid, off: int, n: int, lut_data, lut_valid, lut_n: int, out_data, out_valid,
                          out_bit_offset: int = 0) -> None:
        check(self.handle, lib.ah_is_in_dict_gather(self.handle, index_width, _ptr(indices), _ptr(valid), off, n, _ptr(lut_data), _ptr(lut_valid),
                                                     lut_n, _ptr(out_data), _ptr(out_valid), out_bit_offset))

    def compare_binary(self, cmpop: int, left, right, n: int, out_bits, out_bit_offset: int = 0) -> None:
        """left / right: (offset_width, byte_width, offsets, data, off, broadcast) — offset_width 4 / 8 for base-binary operands,
        0 for fixed slots of byte_width bytes; broadcast 1 for a scalar (every row reads element off)."""
        lo = _CmpOperand(left[0], left[1], _ptr(left[2]), _ptr(left[3]), left[4], left[5])
        ro = _CmpOperand(right[0], right[1], _ptr(right[2]), _ptr(right[3]), right[4], right[5])
        check(self.handle, lib.ah_compare_binary(self.handle, cmpop, C.byref(lo), C.byref(ro), n, _ptr(out_bits), out_bit_offset))

    # ---- string predicates (csrc/ah_string_match.hip, include/arrowhip_strings.h).  column: (offset_width, byte_width, offsets, data, off) — offset_width 4 / 8; 0 (fixed
    # slots of byte_width bytes) only for string_length without utf8.  pattern / program: bytes on the host.
    @staticmethod
    def _column(column) -> _CmpOperand:
        return _CmpOperand(column[0], column[1], _ptr(column[2]), _ptr(column[3]), column[4], 0)

    def string_match(self, op: int, column, n: int, pattern: bytes, out_bits, out_bit_offset: int = 0) -> None:
        """op 0 the pattern occurs in the row, 1 the row starts with it, 2 ends with it, 3 is it: bits [out_bit_offset, + n) of
        out_bits, every other bit kept; every row computed, nulls included; no synchronisation (ah_string_match)"""
        col = self._column(column)
        check(self.handle, lib.ah_string_match(self.handle, op, C.byref(col), n, C.c_char_p(bytes(pattern)), len(pattern), _ptr(out_bits), out_bit_offset))

    def string_find(self, column, n: int, pattern: bytes, out_width: int, out) -> None:
        """out[i] (Int32 / Int64 by out_width) = the byte index of the pattern's first occurrence in row i, -1 for none (ah_string_find)"""
        col = self._column(column)
        check(self.handle, lib.ah_string_find(self.handle, C.byref(col), n, C.c_char_p(bytes(pattern)), len(pattern), out_width, _ptr(out)))

    def string_like(self, column, n: int, utf8: bool, program: bytes, out_bits, out_bit_offset: int = 0) -> None:
        """SQL LIKE with the pattern compiled by compute.like_compile; utf8: `_` is one code point, else one byte (ah_string_like)"""
        col = self._column(column)
        check(self.handle, lib.ah_string_like(self.handle, C.byref(col), n, int(bool(utf8)), C.c_char_p(bytes(program)), len(program), _ptr(out_bits),
                                              out_bit_offset))

    def string_length(self, column, n: int, utf8: bool, out_width: int, out) -> None:
        """out[i] = the bytes of row i, or (utf8) its bytes that are not 10xxxxxx continuation bytes (ah_string_length)"""
        col = self._column(column)
        check(self.handle, lib.ah_string_length(self.handle, C.byref(col), n, int(bool(utf8)), out_width, _ptr(out)))

    # ---- string transforms (csrc/ah_string_transform.hip, include/arrowhip_strings.h).
    # column as above, offset_width 4 / 8; out_starts / out_offsets hold values of that width.
    def string_ranges(self, op: int, column, n: int, out_starts, out_offsets, *, start: int = 0, stop=None, sides: int = 3, chars: bytes = b"",
                      valid=None, valid_offset: int = 0) -> int:
        """op 0 the whole row, 1 / 2 row[start:stop] over bytes / code points (stop None: to the row's end), 3 / 4 the bytes / code
        points of `chars` trimmed from `sides` (1 left, 2 right): out_starts[i] = where row i's result starts in the column's data,
        out_offsets[0 … n] the output offsets; a row whose validity bit (valid_offset + i of `valid`) is clear has length 0.
        Returns the byte total — the call's one synchronisation (ah_string_ranges)"""
        col = self._column(column)
        total = C.c_int64(0)
        check(self.handle, lib.ah_string_ranges(self.handle, op, start, 0 if stop is None else stop, int(stop is not None), sides,
                                                                 C.c_char_p(bytes(chars)), len(chars), C.byref(col), _ptr(valid), valid_offset, n,
                                                                 _ptr(out_starts), _ptr(out_offsets), C.byref(total)))
        return total.value

    def string_gather(self, column, starts, out_offsets, n: int, out_data, map: Optional[bytes] = None) -> None:
        """out_data[out_offsets[i] … out_offsets[i + 1]) = the column's data bytes from starts[i] on, through the 256-byte `map` where
        one is given; no synchronisation (ah_string_gather)"""
        col = self._column(column)
        assert map is None or len(map) == 256
        check(self.handle, lib.ah_string_gather(self.handle, C.byref(col), _ptr(starts), _ptr(out_offsets), n,
                                                                 None if map is None else C.c_char_p(bytes(map)), _ptr(out_data)))

    def compare_decimal(self, cmpop: int, left, right, n: int, out_bits, out_bit_offset: int = 0) -> None:
        """left / right: (width 16 | 32, data, off, broadcast, scale-up exponent)"""
        lw, ld, loff, lb, lk = left
        rw, rd, roff, rb, rk = right
        check(self.handle, lib.ah_compare_decimal(self.handle, cmpop, lw, _ptr(ld), loff, lb, lk, rw, _ptr(rd), roff, rb, rk, n, _ptr(out_bits),
                                                  out_bit_offset))

    # ---- min / max ----------------------------------------------------------------------
    def min_max(self, type_id: int, values, n: int, dtype):
        lo, hi = np.zeros(1, dtype), np.zeros(1, dtype)
        check(self.handle, lib.ah_min_max(self.handle, type_id, _ptr(values), n, lo.ctypes.data, hi.ctypes.data))
        return lo[0], hi[0]

    # ---- sort ---------------------------------------------------------------------------
    def sort_indices(self, type_id: int, values, valid, off: int, n: int, descending: bool, nulls_at_start: bool, out_indices) -> None:
        check(self.handle, lib.ah_sort_indices(self.handle, type_id, _ptr(values), _ptr(valid), off, n, int(descending), int(nulls_at_start),
                                               _ptr(out_indices)))

    def sort_indices_multi(self, keys, n: int, out_indices) -> None:
        """keys: [(type_id, values, valid, off, descending, nulls_at_start), …] — most significant first"""
        k = len(keys)
        types = (C.c_int * k)(*[x[0] for x in keys])
        vals = (C.c_void_p * k)(*[_ptr(x[1]) for x in keys])
        valids = (C.c_void_p * k)(*[_ptr(x[2]) for x in keys])
        offs = (C.c_int64 * k)(*[x[3] for x in keys])
        desc = (C.c_int * k)(*[int(x[4]) for x in keys])
        nfirst = (C.c_int * k)(*[int(x[5]) for x in keys])
        check(self.handle, lib.ah_sort_indices_multi(self.handle, k, types, vals, valids, offs, n, desc, nfirst, _ptr(out_indices)))

    def sort_indices_keys(self, keys, n: int, out_indices) -> None:
        """keys: [(type_id, values, offsets, byte_width, valid, off, descending, nulls_at_start), …] — most significant first; row i
        is element off + i of every buffer (ah_sort_key, include/arrowhip.h)"""
        arr = (SortKey * len(keys))()
        for s, (t, v, o, w, m, off, d, nf) in zip(arr, keys):
            s.type, s.values, s.offsets, s.byte_width, s.valid, s.off = t, _ptr(v), _ptr(o), w, _ptr(m), off
            s.descending, s.nulls_at_start = int(d), int(nf)
        check(self.handle, lib.ah_sort_indices_keys(self.handle, len(keys), arr, n, _ptr(out_indices)))

    def select_k(self, keys, n: int, k: int, out_indices, route: int = 0) -> None:
        """the first min(k, n) entries sort_indices_keys gives for the same keys, into out_indices (ah_select_k); route: 0 auto,
        1 the radix route (a numeric first key), 2 the sort with its final widening cut at k entries"""
        arr = (SortKey * len(keys))()
        for s, (t, v, o, w, m, off, d, nf) in zip(arr, keys):
            s.type, s.values, s.offsets, s.byte_width, s.valid, s.off = t, _ptr(v), _ptr(o), w, _ptr(m), off
            s.descending, s.nulls_at_start = int(d), int(nf)
        check(self.handle, lib.ah_select_k(self.handle, len(keys), arr, n, k, route, _ptr(out_indices)))

    # ---- window functions (ah_window.hip): enqueued on the compute stream, no synchronisation ------------
    def window_flags(self, part_ids, keys, order, n: int, out_flags) -> None:
        """out_flags[p] for every sorted position p (row order[p]; order None: the identity): bit 0 a partition starts (part_ids:
        int32 by row, or None = one partition), bit 1 a peer group starts (the rows do not tie on the keys, laid out as for
        sort_indices_keys; descending / nulls_at_start are not looked at) (ah_window_flags)"""
        arr = (SortKey * max(len(keys), 1))()
        for s, (t, v, o, w, m, off, d, nf) in zip(arr, keys):
            s.type, s.values, s.offsets, s.byte_width, s.valid, s.off = t, _ptr(v), _ptr(o), w, _ptr(m), off
            s.descending, s.nulls_at_start = int(d), int(nf)
        check(self.handle, lib.ah_window_flags(self.handle, _ptr(part_ids), len(keys), arr, _ptr(order), n, _ptr(out_flags)))

    def window_rank(self, kind: int, flags, order, n: int, out) -> None:
        """out[order[p]] (uint64) = kind 0 row_number, 1 rank, 2 dense_rank at sorted position p (ah_window_rank)"""
        check(self.handle, lib.ah_window_rank(self.handle, kind, _ptr(flags), _ptr(order), n, _ptr(out)))

    def window_scan(self, op: int, type_id: int, values, valid, off: int, flags, order, n: int, out_values) -> None:
        """out_values[order[p]] = the running op (0 sum, 1 min, 2 max, 3 count) of the column over its partition up to sorted
        position p; a null row gets payload 0 and the caller copies the validity (ah_window_scan)"""
        check(self.handle, lib.ah_window_scan(self.handle, op, type_id, _ptr(values), _ptr(valid), off, _ptr(flags), _ptr(order), n, _ptr(out_values)))

    # ---- conditionals (ah_conditional.hip).  A side: (offset_width, byte_width, offsets, data, valid, off, broadcast) — offset_width 0
    # for fixed slots of byte_width bytes and for Boolean sides (data a bitmap), 4 / 8 for var-length sides; broadcast 1: a scalar as a
    # one-row device column, every row reads element off.  cond_data / cond_valid: bitmaps read at bit cond_off + row.
    def if_else(self, cond_data, cond_valid, cond_off: int, left, right, n: int, out_values, out_valid) -> None:
        """fixed-width sides: row i = left[i] where cond[i] else right[i], null where cond[i] or the chosen side is (payload 0);
        no synchronisation (ah_if_else)"""
        lo, ro = _cond_side(left), _cond_side(right)
        check(self.handle, lib.ah_if_else(self.handle, _ptr(cond_data), _ptr(cond_valid), cond_off, C.byref(lo), C.byref(ro), n, _ptr(out_values),
                                          _ptr(out_valid)))

    def if_else_boolean(self, cond_data, cond_valid, cond_off: int, left, right, n: int, out_data, out_valid) -> None:
        """Boolean sides: data and validity bitmaps from bit 0 (ah_if_else_boolean)"""
        lo, ro = _cond_side(left), _cond_side(right)
        check(self.handle, lib.ah_if_else_boolean(self.handle, _ptr(cond_data), _ptr(cond_valid), cond_off, C.byref(lo), C.byref(ro), n,
                                                  _ptr(out_data), _ptr(out_valid)))

    def if_else_binary_offsets(self, cond_data, cond_valid, cond_off: int, left, right, n: int, out_offset_width: int, out_offsets,
                               out_valid) -> int:
        """var-length sides, first call: out_offsets[0 … n] and the validity → the number of data bytes (ah_if_else_binary_offsets)"""
        lo, ro = _cond_side(left), _cond_side(right)
        total = C.c_int64()
        check(self.handle, lib.ah_if_else_binary_offsets(self.handle, _ptr(cond_data), _ptr(cond_valid), cond_off, C.byref(lo), C.byref(ro), n,
                                                         out_offset_width, _ptr(out_offsets), _ptr(out_valid), C.byref(total)))
        return total.value

    def if_else_binary_data(self, cond_data, cond_valid, cond_off: int, left, right, n: int, out_offset_width: int, out_offsets,
                            out_data) -> None:
        """var-length sides, second call: the bytes (ah_if_else_binary_data)"""
        lo, ro = _cond_side(left), _cond_side(right)
        check(self.handle, lib.ah_if_else_binary_data(self.handle, _ptr(cond_data), _ptr(cond_valid), cond_off, C.byref(lo), C.byref(ro), n,
                                                      out_offset_width, _ptr(out_offsets), _ptr(out_data)))

    def fill_null_indices(self, valid, off: int, n: int, direction: int, out_idx, out_idx_valid, want_null_count: bool = True):
        """out_idx[i] (uint32) = the nearest valid row at or before (direction 0) / at or after (1) row i, out_idx_valid its bit: what
        the Take family reads as (idx, ivalid).  → the null count, or None without the synchronisation (ah_fill_null_indices)"""
        nulls = C.c_int64()
        check(self.handle, lib.ah_fill_null_indices(self.handle, _ptr(valid), off, n, direction, _ptr(out_idx), _ptr(out_idx_valid),
                                                    C.byref(nulls) if want_null_count else None))
        return nulls.value if want_null_count else None

    def fill_null_directed(self, byte_width: int, values, valid, off: int, n: int, direction: int, out_values, out_valid,
                           want_null_count: bool = True):
        """the same walk with the gather fused in, for values of 1 / 2 / 4 / 8 / 16 / 32 bytes: out_values[i] = values[off + source]
        (ah_fill_null_directed)"""
        nulls = C.c_int64()
        check(self.handle, lib.ah_fill_null_directed(self.handle, byte_width, _ptr(values), _ptr(valid), off, n, direction, _ptr(out_values),
                                                     _ptr(out_valid), C.byref(nulls) if want_null_count else None))
        return nulls.value if want_null_count else None

    def take_boolean(self, data, vvalid, voff: int, nvalues: int, idx_byte_width: int, idx_signed: bool, idx, ivalid, ioff: int, nidx: int,
                     out_data, out_valid) -> int:
        r, bad = C.c_int64(), C.c_int64()
        check(self.handle, lib.ah_take_boolean(self.handle, _ptr(data), _ptr(vvalid), voff, nvalues, idx_byte_width, int(idx_signed), _ptr(idx),
                                               _ptr(ivalid), ioff, nidx, 1, _ptr(out_data), _ptr(out_valid), C.byref(r), C.byref(bad)))
        return r.value

    # ---- var-length take ------------------------------------------------------------------
    def take_binary_offsets(self, offset_width: int, offsets, vvalid, voff: int, nvalues: int, idx_byte_width: int, idx_signed: bool,
                            idx, ivalid, ioff: int, nidx: int, out_offsets, out_valid):
        """→ (null_count, total_bytes)"""
        nulls, total, bad = C.c_int64(), C.c_int64(), C.c_int64()
        check(self.handle, lib.ah_take_binary_offsets(self.handle, offset_width, _ptr(offsets), _ptr(vvalid), voff, nvalues, idx_byte_width,
                                                      int(idx_signed), _ptr(idx), _ptr(ivalid), ioff, nidx, 1, _ptr(out_offsets),
                                                      _ptr(out_valid), C.byref(nulls), C.byref(total), C.byref(bad)))
        return nulls.value, total.value

    def take_binary_data(self, offset_width: int, offsets, data, voff: int, idx_byte_width: int, idx, nidx: int, out_offsets, out_data) -> None:
        check(self.handle, lib.ah_take_binary_data(self.handle, offset_width, _ptr(offsets), _ptr(data), voff, idx_byte_width, _ptr(idx), nidx,
                                                   _ptr(out_offsets), _ptr(out_data)))

    # ---- hashing ------------------------------------------------------------------------
    def hash_u64_encode(self, keys, valid, off: int, n: int, encode_nulls: bool, out_ids, out_ids_valid, out_dict):
        nd = C.c_int64()
        nid = C.c_int32()
        check(self.handle, lib.ah_hash_u64_encode(self.handle, _ptr(keys), _ptr(valid), off, n, int(encode_nulls), _ptr(out_ids),
                                                  _ptr(out_ids_valid), _ptr(out_dict), C.byref(nd), C.byref(nid)))
        return nd.value, nid.value

    def hash_binary_encode(self, offset_width: int, offsets, data, valid, off: int, n: int, encode_nulls: bool, out_ids, out_ids_valid,
                           out_first_rows):
        nd = C.c_int64()
        nid = C.c_int32()
        check(self.handle, lib.ah_hash_binary_encode(self.handle, offset_width, _ptr(offsets), _ptr(data), _ptr(valid), off, n,
                                                     int(encode_nulls), _ptr(out_ids), _ptr(out_ids_valid), _ptr(out_first_rows),
                                                     C.byref(nd), C.byref(nid)))
        return nd.value, nid.value

    def hash_fixed_encode(self, byte_width: int, data, valid, off: int, n: int, encode_nulls: bool, out_ids, out_ids_valid, out_first_rows, out_dict):
        nd = C.c_int64()
        nid = C.c_int32()
        check(self.handle, lib.ah_hash_fixed_encode(self.handle, byte_width, _ptr(data), _ptr(valid), off, n, int(encode_nulls), _ptr(out_ids),
                                                    _ptr(out_ids_valid), _ptr(out_first_rows), _ptr(out_dict), C.byref(nd), C.byref(nid)))
        return nd.value, nid.value

    def hash_sum(self, kind: str, keys, kvalid, koff: int, vals, vvalid, voff: int, n: int, out_keys, out_sums, out_counts,
                 out_first_rows=None):
        ng = C.c_int64()
        nid = C.c_int32()
        fn = lib.ah_hash_sum_f64 if kind == "f64" else lib.ah_hash_sum_i64
        check(self.handle, fn(self.handle, _ptr(keys), _ptr(kvalid), koff, _ptr(vals), _ptr(vvalid), voff, n, _ptr(out_keys),
                              _ptr(out_sums), _ptr(out_counts), _ptr(out_first_rows), C.byref(ng), C.byref(nid)))
        return ng.value, nid.value

    def hash_min_max(self, kind: str, keys, kvalid, koff: int, vals, vvalid, voff: int, n: int, out_keys, out_mins, out_maxs, out_counts,
                     out_first_rows=None):
        """group-by min / max of 8-byte values (kind "i64" signed, "u64" unsigned, "f64": NaNs ignored, -0 < +0) over the groups of
        hash_sum; a group with count 0 holds zero bytes.  Returns (ngroups, null_group)."""
        fns = {"i64": lib.ah_hash_min_max_i64, "u64": lib.ah_hash_min_max_u64, "f64": lib.ah_hash_min_max_f64}
        if kind not in fns:
            raise ValueError(f"hash_min_max: kind must be one of 'i64', 'u64', 'f64', not {kind!r}")
        ng = C.c_int64()
        nid = C.c_int32()
        check(self.handle, fns[kind](self.handle, _ptr(keys), _ptr(kvalid), koff, _ptr(vals), _ptr(vvalid), voff, n, _ptr(out_keys),
                                     _ptr(out_mins), _ptr(out_maxs), _ptr(out_counts), _ptr(out_first_rows), C.byref(ng), C.byref(nid)))
        return ng.value, nid.value

    def group_ids(self, keys, n: int, out_ids, out_first_rows) -> int:
        """dense first-seen group ids of a tuple of 1 … 8 key columns; keys: [(offset_width, byte_width, bits, offsets, data, valid, off),
        …] — offset_width 4 / 8: String / Binary (Large…), byte_width 1 … 4096: fixed slots, bits 1: Boolean; row i is element off + i
        of every buffer (ah_group_key, include/arrowhip.h).  A null is a value of its column.  out_ids: n int32, out_first_rows: int64,
        n + 1 entries of room.  Returns the number of groups."""
        arr = (GroupKey * max(len(keys), 1))()
        for s, (ow, bw, bits, offsets, data, valid, off) in zip(arr, keys):
            s.offset_width, s.byte_width, s.bits, s.offsets, s.data, s.valid, s.off = ow, bw, int(bits), _ptr(offsets), _ptr(data), _ptr(valid), off
        ng = C.c_int64()
        check(self.handle, lib.ah_group_ids(self.handle, len(keys), arr, n, _ptr(out_ids), _ptr(out_first_rows), C.byref(ng)))
        return ng.value

    def group_sum(self, kind: str, ids, ngroups: int, vals, vvalid, voff: int, n: int, out_sums, out_counts) -> None:
        """hash_sum's sums and counts over caller-supplied dense ids (0 <= ids[i] < ngroups: not checked); kind: "i64" (wrapping) or "f64" (the fixed-point sum)"""
        fns = {"i64": lib.ah_group_sum_i64, "f64": lib.ah_group_sum_f64}
        if kind not in fns:
            raise ValueError(f"group_sum: kind must be one of 'i64', 'f64', not {kind!r}")
        check(self.handle, fns[kind](self.handle, _ptr(ids), ngroups, _ptr(vals), _ptr(vvalid), voff, n, _ptr(out_sums), _ptr(out_counts)))

    def group_min_max(self, kind: str, ids, ngroups: int, vals, vvalid, voff: int, n: int, out_mins, out_maxs, out_counts) -> None:
        """hash_min_max's minima, maxima and counts over caller-supplied dense ids (0 <= ids[i] < ngroups: not checked)"""
        fns = {"i64": lib.ah_group_min_max_i64, "u64": lib.ah_group_min_max_u64, "f64": lib.ah_group_min_max_f64}
        if kind not in fns:
            raise ValueError(f"group_min_max: kind must be one of 'i64', 'u64', 'f64', not {kind!r}")
        check(self.handle, fns[kind](self.handle, _ptr(ids), ngroups, _ptr(vals), _ptr(vvalid), voff, n, _ptr(out_mins), _ptr(out_maxs),
                                     _ptr(out_counts)))

    def group_count(self, ids, ngroups: int, vvalid, voff: int, n: int, out_counts) -> None:
        """rows of every group whose validity bit is set (vvalid None: every row) into out_counts (ngroups int64); reads no values"""
        check(self.handle, lib.ah_group_count(self.handle, _ptr(ids), ngroups, _ptr(vvalid), voff, n, _ptr(out_counts)))

    def group_sum_typed(self, type_id: int, ids, ngroups: int, vals, vvalid, voff: int, n: int, out_sums, out_counts) -> None:
        """group_sum for a value column of any numeric type id (AH_INT8 ... AH_FLOAT64), read at its own width: out_sums holds ngroups
        8-byte sums — wrapping Int64 (signed), wrapping UInt64 (unsigned), Float64 (floats) — with the bytes of group_sum on the cast column"""
        check(self.handle, lib.ah_group_sum_typed(self.handle, type_id, _ptr(ids), ngroups, _ptr(vals), _ptr(vvalid), voff, n, _ptr(out_sums),
                                                  _ptr(out_counts)))

    def group_min_max_typed(self, type_id: int, ids, ngroups: int, vals, vvalid, voff: int, n: int, out_mins, out_maxs, out_counts) -> None:
        """group_min_max for a value column of any numeric type id; out_mins / out_maxs hold ngroups values of the input type"""
        check(self.handle, lib.ah_group_min_max_typed(self.handle, type_id, _ptr(ids), ngroups, _ptr(vals), _ptr(vvalid), voff, n, _ptr(out_mins),
                                                      _ptr(out_maxs), _ptr(out_counts)))

    def group_mean(self, sum_type: int, sums, counts, ngroups: int, out_means) -> None:
        """out_means[g] = float64(sums[g]) / float64(counts[g]), 0.0 where the count is 0; sum_type: AH_INT64, AH_UINT64 or AH_FLOAT64"""
        check(self.handle, lib.ah_group_mean(self.handle, sum_type, _ptr(sums), _ptr(counts), ngroups, _ptr(out_means)))

    def group_m2(self, type_id: int, ids, ngroups: int, vals, vvalid, voff: int, n: int, out_means, out_m2, out_counts) -> None:
        """means, sums of squared deviations from the mean and valid counts (ngroups float64 / float64 / int64) of a value column of any
        numeric type id, read at its own width and taken as cast to float64; the bytes are the same on every run and launch geometry"""
        check(self.handle, lib.ah_group_m2(self.handle, type_id, _ptr(ids), ngroups, _ptr(vals), _ptr(vvalid), voff, n, _ptr(out_means),
                                           _ptr(out_m2), _ptr(out_counts)))

    def group_variance(self, m2, counts, ngroups: int, ddof: int, take_sqrt: bool, out) -> None:
        """out[g] = m2[g] / float64(counts[g] - ddof), its square root with take_sqrt; 0.0 where counts[g] <= ddof"""
        check(self.handle, lib.ah_group_variance(self.handle, _ptr(m2), _ptr(counts), ngroups, ddof, 1 if take_sqrt else 0, _ptr(out)))

    # ---- hash join over dense group ids (ah_join.hip): ids int32, row numbers / starts / offsets int64, validity = bit off + row -----------
    def join_build(self, build_ids, build_valid, voff: int, n_build: int, ngroups: int, out_starts, out_rows) -> None:
        """out_starts[g] .. out_starts[g + 1] (ngroups + 1 entries) delimit, in out_rows (n_build entries of room), the valid build rows
        of group g in ascending row order"""
        check(self.handle, lib.ah_join_build(self.handle, _ptr(build_ids), _ptr(build_valid), voff, n_build, ngroups, _ptr(out_starts), _ptr(out_rows)))

    def join_count(self, probe_ids, probe_valid, poff: int, n_probe: int, starts, emit_unmatched: bool, out_offsets) -> int:
        """out_offsets (n_probe + 1 entries) = the exclusive scan of every probe row's match count (at least 1 with emit_unmatched);
        returns the total, the rows of the join's result"""
        total = C.c_int64()
        check(self.handle, lib.ah_join_count(self.handle, _ptr(probe_ids), _ptr(probe_valid), poff, n_probe, _ptr(starts), int(bool(emit_unmatched)),
                                             _ptr(out_offsets), C.byref(total)))
        return total.value

    def join_expand(self, probe_ids, probe_valid, poff: int, n_probe: int, starts, rows, offsets, total: int, emit_unmatched: bool,
                    out_probe_rows, out_build_rows, out_build_valid=None) -> int:
        """the probe row and the build row of every output slot (`total` int64 entries each); with emit_unmatched also the validity
        bitmap of the build rows, and the number of its clear bits is returned (0 without)"""
        nulls = C.c_int64()
        check(self.handle, lib.ah_join_expand(self.handle, _ptr(probe_ids), _ptr(probe_valid), poff, n_probe, _ptr(starts), _ptr(rows), _ptr(offsets),
                                              total, int(bool(emit_unmatched)), _ptr(out_probe_rows), _ptr(out_build_rows), _ptr(out_build_valid),
                                              C.byref(nulls)))
        return nulls.value

    def join_match_bits(self, probe_ids, probe_valid, poff: int, n_probe: int, starts, out_bits) -> None:
        """bit i of out_bits = probe row i is valid and its group holds a build row (the mask of a semi join)"""
        check(self.handle, lib.ah_join_match_bits(self.handle, _ptr(probe_ids), _ptr(probe_valid), poff, n_probe, _ptr(starts), _ptr(out_bits)))

    def lz4_decompress_blocks(self, src, src_bytes: int, dst, dst_bytes: int, blocks):
        """independent LZ4 blocks of the device bytes `src` inflated into the device bytes `dst`; blocks: rows of {src_off, src_len
        (bit 62: stored), dst_off, dst_len <= 65536}, dst_off ascending.  Returns the status byte of every block as a numpy array
        (0 ok, 1 corrupt, 2 produced != dst_len); a block with a status leaves unspecified bytes in its own output range only."""
        table = np.ascontiguousarray(np.asarray(blocks, np.int64).reshape(-1, 4))
        status = np.zeros(len(table), np.uint8)
        nbad = C.c_int64()
        check(self.handle, lib.ah_lz4_decompress_blocks(self.handle, _ptr(src), src_bytes, _ptr(dst), dst_bytes, table.ctypes.data, len(table),
                                                        status.ctypes.data, C.byref(nbad)))
        assert nbad.value == int(np.count_nonzero(status))
        return status

    def lz4_compress_blocks(self, src, src_bytes: int, dst, dst_bytes: int, blocks):
        """blocks of at most 65536 device bytes of `src`, each compressed on its own as one LZ4 block into its slot of `dst`; blocks:
        rows of {src_off, src_len, dst_off}, the slots dst[dst_off, dst_off + src_len) ascending without overlap.  Returns (sizes,
        stored) as numpy arrays: the bytes written to each slot, and 1 where the block did not shrink and its slot holds the input."""
        table = np.ascontiguousarray(np.asarray(blocks, np.int64).reshape(-1, 3))
        sizes = np.zeros(len(table), np.int32)
        stored = np.zeros(len(table), np.uint8)
        check(self.handle, lib.ah_lz4_compress_blocks(self.handle, _ptr(src), src_bytes, _ptr(dst), dst_bytes, table.ctypes.data, len(table),
                                                      sizes.ctypes.data, stored.ctypes.data))
        return sizes, stored

    def ipc_pack_body(self, comp, comp_bytes: int, plain, plain_bytes: int, lits: bytes, rows, dst, dst_bytes: int) -> None:
        """dst[0, dst_bytes) := the pieces of `rows` {src_off, len, dst_off, word} end to end; word & 3: 0 the device bytes `comp`, 1 the
        device bytes `plain`, 2 the host bytes `lits`; word bit 8: the 32 bits above bit 32 go, little-endian, in front of the piece.
        The rows must tile the output exactly."""
        table = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, 4))
        lit = np.frombuffer(bytes(lits), np.uint8)
        check(self.handle, lib.ah_ipc_pack_body(self.handle, _ptr(comp), comp_bytes, _ptr(plain), plain_bytes, lit.ctypes.data if len(lit) else None,
                                                len(lit), table.ctypes.data if len(table) else None, len(table), _ptr(dst), dst_bytes))

    def hash_partition(self, keys, n: int, nparts: int, out_part) -> None:
        check(self.handle, lib.ah_hash_partition_u64(self.handle, _ptr(keys), n, nparts, _ptr(out_part)))

    # ---- fused expressions --------------------------------------------------------------
    def expr_compile(self, nodes, col_types, lit_types):
        """nodes: [(opcode, arg), …] postfix.  Returns (handle, out_type)."""
        na = _nodes_array(nodes)
        ct = (C.c_int * max(len(col_types), 1))(*col_types)
        lt = (C.c_int * max(len(lit_types), 1))(*lit_types)
        h = C.c_void_p()
        ot = C.c_int()
        check(self.handle, lib.ah_expr_compile(self.handle, na, len(nodes), ct, len(col_types), lt, len(lit_types), C.byref(h), C.byref(ot)))
        return h, ot.value

    def expr_execute(self, handle, col_values, col_valid, col_offsets, lit_values, lit_valid, n: int, out_values, out_valid) -> None:
        nc = max(len(col_values), 1)
        cv = (C.c_void_p * nc)(*[_ptr(x) for x in col_values])
        cvd = (C.c_void_p * nc)(*[_ptr(x) for x in col_valid])
        co = (C.c_int64 * nc)(*col_offsets)
        nl = max(len(lit_values), 1)
        lv = (C.c_uint8 * (8 * nl))()
        for i, raw in enumerate(lit_values):  # raw: bytes (≤ 8) little-endian payload
            C.memmove(C.addressof(lv) + 8 * i, raw, len(raw))
        lvd = (C.c_int * nl)(*[int(x) for x in lit_valid]) if lit_valid else (C.c_int * nl)()
        check(self.handle, lib.ah_expr_execute(self.handle, handle, cv, cvd, co, lv, lvd, n, _ptr(out_values), _ptr(out_valid)))

    def expr_source(self, handle) -> str:
        return lib.ah_expr_source(handle).decode()

    # ---- fused --------------------------------------------------------------------------
    def cmp_filter_sum_i64(self, cmpop: int, x, valid, off: int, n: int, threshold: int):
        s = C.c_int64()
        cnt = C.c_int64()
        check(self.handle, lib.ah_cmp_filter_sum_i64(self.handle, cmpop, _ptr(x), _ptr(valid), off, n, threshold, C.byref(s), C.byref(cnt)))
        return s.value, cnt.value

    def cmp_filter_sum_f64(self, cmpop: int, x, valid, off: int, n: int, threshold: float):
        s = C.c_double()
        cnt = C.c_int64()
        check(self.handle, lib.ah_cmp_filter_sum_f64(self.handle, cmpop, _ptr(x), _ptr(valid), off, n, threshold, C.byref(s), C.byref(cnt)))
        return s.value, cnt.value

    def cmp_filter_sum_i64_dev(self, cmpop: int, x, valid, off: int, n: int, threshold: int, out_sum_count_dev) -> None:
        check(self.handle, lib.ah_cmp_filter_sum_i64_dev(self.handle, cmpop, _ptr(x), _ptr(valid), off, n, threshold,
                                                         _ptr(out_sum_count_dev)))

    def cmp_filter_sum_f64_dev(self, cmpop: int, x, valid, off: int, n: int, threshold: float, out_sum_dev, out_count_dev) -> None:
        check(self.handle, lib.ah_cmp_filter_sum_f64_dev(self.handle, cmpop, _ptr(x), _ptr(valid), off, n, threshold,
                                                         _ptr(out_sum_dev), _ptr(out_count_dev)))


def _nodes_array(nodes):
    arr = (C.c_int32 * (2 * len(nodes)))()
    for i, (op, arg) in enumerate(nodes):
        arr[2 * i], arr[2 * i + 1] = op, arg
    return arr


def expr_codegen(nodes, col_types, lit_types, compile_it: bool = True):
    """Stateless: generate (and hiprtc-compile for gfx950) the fused kernel of a postfix
    program; works without a GPU.  Returns (source, out_type); raises on error."""
    na = _nodes_array(nodes)
    ct = (C.c_int * max(len(col_types), 1))(*col_types)
    lt = (C.c_int * max(len(lit_types), 1))(*lit_types)
    src = C.create_string_buffer(1 << 16)
    err = C.create_string_buffer(1024)
    ot = C.c_int()
    st = lib.ah_expr_codegen(na, len(nodes), ct, len(col_types), lt, len(lit_types), int(compile_it), src, len(src), err, len(err),
                             C.byref(ot))
    if st != N.AH_OK:
        raise N._ERRS.get(st, N.ArrowHipError)(err.value.decode())
    return src.value.decode(), ot.value


def device_count() -> int:
    n = C.c_int()
    st = lib.ah_device_count(C.byref(n))
    return n.value if st == N.AH_OK else 0
