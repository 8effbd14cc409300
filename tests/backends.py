"""Two implementations of the same leaf interface, so every parity test body runs
unchanged against (a) the CPU oracle and (b) the HIP library through the C ABI.

  OracleBackend — oracle/liboracle.so (checker; `-m "not gpu"` pins it to the
                  reference's golden vectors)
  HipBackend    — libarrowhip.so on cuda:0 through include/arrowhip.h (`-m gpu`)

All inputs/outputs are host numpy arrays; HipBackend uploads, runs, downloads.
`misalign` (elements) shifts the device copy of a value buffer off 16-byte alignment
the way an Arrow slice (&values[offset]) does: every value input and the output together.
`misalign_l=` / `misalign_r=` / `misalign_in=` / `misalign_idx=` … shift one input on its
own, `out_phase=` (bytes, a multiple of the element width) places the output alone.

Every HipBackend output is a GuardedBuffer: exactly the bytes include/arrowhip.h gives
the output, between two 4 KiB bands that must come back unchanged — after a successful
call and after one that returned AH_EOVERFLOW / AH_EINVALID / AH_EINDEX.
"""
from __future__ import annotations

import numpy as np

from arrow_go_amd.device import DeviceBuffer
from tests import oracle_lib as OL

STATUS_OK, STATUS_EINVALID, STATUS_EINDEX, STATUS_EOVERFLOW = 0, 1, 2, 3

GUARD_BAND = 4096   # bytes on each side: more than a whole wave's 64 × 16-byte store
GUARD_FILL = 0x5A   # no payload fill of the suite (0x00, 0xFF, 0xA5, 0xCD)


class GuardedBuffer(DeviceBuffer):
    """One allocation laid out as  front band | lead | payload | back band.

    `ptr` is the first payload byte and `nbytes` the payload's size: upload / download / memset offsets are relative to the
    payload, so a GuardedBuffer stands wherever a DeviceBuffer does.  The allocation's base is 256-byte aligned, so the payload
    sits at phase `lead % 16` of a 16-byte line.  check() reads both bands back and names the first changed byte.

    `ctx` needs alloc(nbytes) → an object with ptr / upload / download / memset / free (arrow_go_amd.Context, or a stand-in)."""

    def __init__(self, ctx, nbytes: int, lead: int = 0, name: str = "output"):
        assert nbytes >= 0 and lead >= 0
        self.ctx = ctx
        self.nbytes = int(nbytes)
        self.lead = int(lead)
        self.name = name
        self._off = GUARD_BAND + self.lead
        self._raw = ctx.alloc(self._off + self.nbytes + GUARD_BAND)
        self.base = self._raw.ptr
        assert self.base % 256 == 0, f"allocation base {self.base:#x} is not 256-byte aligned"
        self.ptr = self.base + self._off
        # the lead bytes are band bytes too; the payload is the caller's to fill
        self._raw.memset(GUARD_FILL, self._off, 0)
        self._raw.memset(GUARD_FILL, GUARD_BAND, self._off + self.nbytes)

    def upload(self, arr, byte_offset: int = 0) -> "GuardedBuffer":
        a = np.ascontiguousarray(arr)
        assert 0 <= byte_offset and byte_offset + a.nbytes <= self.nbytes, "upload outside the payload"
        self._raw.upload(a, self._off + byte_offset)
        return self

    def download(self, dtype, count: int, byte_offset: int = 0) -> np.ndarray:
        assert 0 <= byte_offset and byte_offset + int(count) * np.dtype(dtype).itemsize <= self.nbytes, "download outside the payload"
        return self._raw.download(dtype, count, self._off + byte_offset)

    def memset(self, byte_value: int, nbytes=None, byte_offset: int = 0) -> None:
        nbytes = self.nbytes - byte_offset if nbytes is None else nbytes
        assert 0 <= byte_offset and byte_offset + nbytes <= self.nbytes, "memset outside the payload"
        if nbytes:
            self._raw.memset(byte_value, nbytes, self._off + byte_offset)

    def changed(self):
        """→ None, or (side, distance): the changed band byte nearest to the payload's edge on the first side that changed;
        distance 1 is the byte directly in front of / behind the payload"""
        front = self._raw.download(np.uint8, self._off, 0)
        bad = np.flatnonzero(front != GUARD_FILL)
        if bad.size:
            return "front", int(self._off - bad[-1])
        back = self._raw.download(np.uint8, GUARD_BAND, self._off + self.nbytes)
        bad = np.flatnonzero(back != GUARD_FILL)
        if bad.size:
            return "back", int(bad[0]) + 1
        return None

    def check(self, what: str) -> None:
        hit = self.changed()
        if hit is not None:
            side, dist = hit
            where = "in front of the first" if side == "front" else "behind the last"
            raise AssertionError(f"{what}: wrote outside {self.name} ({self.nbytes} bytes at phase {self.lead % 16}): "
                                 f"{side} band changed, nearest byte {dist} {where} payload byte")

    def free(self) -> None:
        if self.ptr:
            self._raw.free()
            self.ptr = 0
            self.base = 0

    def __del__(self):
        try:
            if self.ptr and getattr(self.ctx, "handle", None):
                self.free()
        except Exception:
            pass


class OracleBackend:
    name = "oracle"

    def __init__(self):
        self.o = OL.load_oracle()

    def sum(self, arr, misalign=0):
        arr = np.ascontiguousarray(arr)
        if arr.dtype == np.float64:
            return float(self.o.sum_float64_exact(arr))
        return int(self.o.sum_int64(arr)) if arr.dtype == np.int64 else int(self.o.sum_uint64(arr))

    def arithmetic(self, op, shape, l, r, misalign=0):
        return self.o.arithmetic(op, shape, l, r)

    def arithmetic_unary(self, op, a, misalign=0):
        return self.o.arithmetic_unary(op, a)

    def arithmetic_checked(self, op, shape, l, lvalid, loff, r, rvalid, roff, scalar_valid=True, misalign=0):
        return self.o.arithmetic_checked(op, shape, l, lvalid, loff, r, rvalid, roff, scalar_valid)

    def arithmetic_ext(self, op, shape, l, lvalid, loff, r, rvalid, roff, scalar_valid=True):
        """→ (status, out, error text)"""
        return self.o.arithmetic_ext(op, shape, l, lvalid, loff, r, rvalid, roff, scalar_valid)

    def round(self, values, valid, off, ndigits, mode, multiple=None):
        return self.o.round(values, valid, off, ndigits, mode, multiple)

    def comparison(self, cmpop, shape, l, r, out_init, out_bit_offset=0, misalign=0):
        out = np.array(out_init, dtype=np.uint8, copy=True)
        return self.o.comparison(cmpop, shape, l, r, out, out_bit_offset)

    def count_set_bits(self, bits, off, n):
        return self.o.count_set_bits(np.ascontiguousarray(bits), off, n)

    def bitmap_op(self, op, l, loff, r, roff, out_init, ooff, n):
        return self.o.bitmap_op(op, l, loff, r, roff, np.array(out_init, dtype=np.uint8, copy=True), ooff, n)

    def copy_bitmap(self, src, soff, n, out_init, doff, invert=False):
        return self.o.copy_bitmap(src, soff, n, np.array(out_init, dtype=np.uint8, copy=True), doff, invert)

    def set_bits_to(self, out_init, off, n, value):
        return self.o.set_bits_to(np.array(out_init, dtype=np.uint8, copy=True), off, n, value)

    def kleene(self, op, lvalid, ldata, loff, rvalid, rdata, roff, ovalid_init, odata_init, ooff, n):
        return self.o.kleene(op, lvalid, ldata, loff, rvalid, rdata, roff, np.array(ovalid_init, dtype=np.uint8, copy=True),
                             np.array(odata_init, dtype=np.uint8, copy=True), ooff, n)

    def filter_count(self, fdata, fvalid, foff, n, null_sel):
        return self.o.filter_count(fdata, fvalid, foff, n, null_sel)

    def filter(self, values, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid, misalign=0):
        return self.o.filter_primitive(values, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid)

    def filter_to_indices(self, fdata, fvalid, foff, n, null_sel, want_valid):
        return self.o.filter_to_indices(fdata, fvalid, foff, n, null_sel, want_valid)

    def take(self, values, vvalid, voff, idx, ivalid, ioff, bounds_check, want_valid):
        return self.o.take_primitive(values, vvalid, voff, idx, ivalid, ioff, bounds_check, want_valid)

    def cumulative_sum(self, values, valid, off, start=None, skip_nulls=False, checked=False, misalign=0):
        return self.o.cumulative_sum(values, valid, off, start, skip_nulls, checked)

    def cast_numeric(self, values, out_dtype, valid=None, off=0, allow_int_overflow=False, allow_float_truncate=False, misalign=0):
        return self.o.cast_numeric(values, out_dtype, valid, off, allow_int_overflow, allow_float_truncate)

    def cast_bool_to_numeric(self, bits, off, n, out_dtype):
        return self.o.cast_bool_to_numeric(bits, off, n, out_dtype)

    def shift_time(self, values, out_dtype, op, factor, check, valid=None, off=0, misalign=0):
        return self.o.shift_time(values, out_dtype, op, factor, check, valid, off)

    def is_in(self, values, valid, off, set_values, set_valid, set_off, null_behavior, out_off=0, fill=0, misalign=0):
        return self.o.is_in(values, valid, off, set_values, set_valid, set_off, null_behavior, out_off, fill)

    def sort_indices(self, values, valid, off, descending=False, nulls_at_start=False, misalign=0):
        return self.o.sort_indices(values, valid, off, descending, nulls_at_start)

    def min_max(self, values, misalign=0):
        return self.o.min_max(values)

    def sort_indices_multi(self, columns):
        return self.o.sort_indices_multi(columns)

    def take_binary(self, offsets, data, vvalid, voff, nvalues, idx, ivalid, ioff, want_valid):
        return self.o.take_binary(offsets, data, vvalid, voff, nvalues, idx, ivalid, ioff, want_valid)

    def filter_binary(self, offsets, data, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid):
        return self.o.filter_binary(offsets, data, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid)

    def hash_encode(self, keys, valid, off, encode_nulls):
        return self.o.hash_u64_encode(keys, valid, off, encode_nulls)

    def hash_binary_encode(self, offsets, data, valid, off, n, encode_nulls):
        return self.o.hash_binary_encode(offsets, data, valid, off, n, encode_nulls)

    def hash_fixed_encode(self, data, w, valid, off, n, encode_nulls):
        """fixed-width keys = binary keys whose offsets are implied (i·w): the oracle's binary memo table over explicit offsets"""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = (np.arange(data.size // w + 1, dtype=np.int64) * w)
        ids, idv, first, nid = self.o.hash_binary_encode(offsets, data, valid, off, n, encode_nulls)
        base = data[off * w:].reshape(-1, w)
        dic = np.zeros((first.size, w), np.uint8)
        for i, r in enumerate(first):
            if i != nid:
                dic[i] = base[r]
        return ids, idv, first, nid, dic.reshape(-1)

    def hash_sum(self, kind, keys, kvalid, koff, vals, vvalid, voff):
        return self.o.hash_sum(kind, keys, kvalid, koff, vals, vvalid, voff)

    def cmp_filter_sum_i64(self, cmpop, x, valid, off, thr):
        return self.o.cmp_filter_sum_i64(cmpop, x, valid, off, thr)

    def cmp_filter_sum_f64(self, cmpop, x, valid, off, thr):
        s_seq, s_exact, cnt = self.o.cmp_filter_sum_f64(cmpop, x, valid, off, thr)
        return s_exact, cnt


class HipBackend:
    name = "hip"
    INPUT_PAD = 64   # spare bytes behind an input: the kernels read bitmaps and values by whole aligned words (outputs get none)

    def __init__(self, ctx, dirty_outputs=False):
        self.c = ctx
        self.dirty_outputs = dirty_outputs
        self._guards = []

    # -- helpers
    def _dirty(self, nbytes):
        """a padded input buffer; with dirty_outputs its memory held something else before (0xA5 …), so that a kernel which reads
        behind its input shows.  tests/test_gpu_parity.py runs that way."""
        buf = self.c.alloc(nbytes)
        if self.dirty_outputs:
            buf.memset(0xA5)
        return buf

    def _out(self, name, nbytes, phase=0, fill=None, init=None):
        """an output of exactly `nbytes` owned bytes at byte phase `phase` of a 16-byte line, between guard bands that the next
        _run() checks.  With dirty_outputs the payload held 0xA5 before, so that a kernel which defines only part of its last byte
        shows; `fill` is the byte a test wants there instead, `init` the bytes an in-place (bit offset) output starts from."""
        buf = GuardedBuffer(self.c, nbytes, phase, name)
        if init is not None:
            buf.upload(init)
        elif fill is not None:
            buf.memset(fill)
        elif self.dirty_outputs:
            buf.memset(0xA5)
        else:
            buf.memset(0x00)
        self._guards.append(buf)
        return buf

    def _run(self, what, fn, *args, **kw):
        """call the entry point `what` and check the bands of every output allocated since the last call — also when it returns
        AH_EOVERFLOW / AH_EINVALID / AH_EINDEX: a failed call owns no more than a successful one"""
        import arrow_go_amd as ah
        guards, self._guards = self._guards, []
        try:
            r = fn(*args, **kw)
        except ah.ErrHip:
            raise
        except ah.ArrowHipError:
            for g in guards:
                g.check(what)
            raise
        for g in guards:
            g.check(what)
        return r

    @staticmethod
    def _phase(out_phase, misalign, w):
        """byte phase of an output: its own `out_phase`, or with the inputs (`misalign` elements)"""
        if out_phase is None:
            return misalign * w
        assert out_phase % w == 0, "out_phase must be a multiple of the element width"
        return out_phase

    def _up(self, arr, misalign=0):
        """upload; returns (buffer, device pointer of element 0)"""
        if arr is None:
            return None, None
        a = np.ascontiguousarray(arr)
        lead = misalign * a.dtype.itemsize
        buf = self.c.alloc(lead + a.nbytes + self.INPUT_PAD)
        buf.upload(a, lead)
        return buf, buf.ptr + lead

    def _upbits(self, bits):
        if bits is None:
            return None, None
        a = np.ascontiguousarray(bits, dtype=np.uint8)
        buf = self._dirty(a.nbytes + self.INPUT_PAD)
        buf.upload(a)
        return buf, buf.ptr

    def sum(self, arr, misalign=0):
        arr = np.ascontiguousarray(arr)
        b, p = self._up(arr, misalign)
        if arr.dtype == np.float64:
            return self.c.sum_float64(p, arr.size)
        if arr.dtype == np.int64:
            return self.c.sum_int64(p, arr.size)
        return self.c.sum_uint64(p, arr.size)

    def arithmetic(self, op, shape, l, r, misalign=0, *, misalign_l=None, misalign_r=None, out_phase=None):
        l = np.ascontiguousarray(l); r = np.ascontiguousarray(r)
        arr = r if shape == 2 else l
        tid = OL.TYPE_IDS[arr.dtype]
        lb, lp = (None, l) if shape == 2 else self._up(l, misalign if misalign_l is None else misalign_l)
        rb, rp = (None, r) if shape == 1 else self._up(r, misalign if misalign_r is None else misalign_r)
        ob = self._out("out", arr.nbytes, self._phase(out_phase, misalign, arr.dtype.itemsize))
        self._run(("ah_arithmetic_binary", "ah_arithmetic_arr_scalar", "ah_arithmetic_scalar_arr")[shape],
                  self.c.arithmetic, tid, op, shape, lp, rp, ob, arr.size)
        return ob.download(arr.dtype, arr.size)

    def arithmetic_unary(self, op, a, misalign=0, *, misalign_in=None, out_phase=None):
        a = np.ascontiguousarray(a)
        ib, ip = self._up(a, misalign if misalign_in is None else misalign_in)
        ob = self._out("out", a.nbytes, self._phase(out_phase, misalign, a.dtype.itemsize))
        self._run("ah_arithmetic_unary", self.c.arithmetic_unary, OL.TYPE_IDS[a.dtype], op, ip, ob, a.size)
        return ob.download(a.dtype, a.size)

    def arithmetic_checked(self, op, shape, l, lvalid, loff, r, rvalid, roff, scalar_valid=True, misalign=0, *,
                           misalign_l=None, misalign_r=None, out_phase=None):
        import arrow_go_amd as ah
        l = np.ascontiguousarray(l); r = np.ascontiguousarray(r)
        arr = r if shape == 2 else l
        lb, lp = (None, l) if shape == 2 else self._up(l, misalign if misalign_l is None else misalign_l)
        rb, rp = (None, r) if shape == 1 else self._up(r, misalign if misalign_r is None else misalign_r)
        lvb, lvp = self._upbits(lvalid)
        rvb, rvp = self._upbits(rvalid)
        ob = self._out("out", arr.nbytes, self._phase(out_phase, misalign, arr.dtype.itemsize), fill=0xCD)
        try:
            self._run("ah_arithmetic_checked", self.c.arithmetic_checked, OL.TYPE_IDS[arr.dtype], op, shape, lp, lvp, loff, rp, rvp, roff,
                      scalar_valid, ob, arr.size)
            st = STATUS_OK
        except ah.ErrOverflow as e:
            assert "overflow" in str(e)
            st = STATUS_EOVERFLOW
        return st, ob.download(arr.dtype, arr.size)

    def round(self, values, valid, off, ndigits, mode, multiple=None, *, misalign_in=0, out_phase=0):
        import arrow_go_amd as ah
        values = np.ascontiguousarray(values)
        vb, vp = self._up(values, misalign_in); vvb, vvp = self._upbits(valid)
        ob = self._out("out", values.nbytes, self._phase(out_phase, 0, values.dtype.itemsize), fill=0xCD)
        m = None if multiple is None else np.array([multiple], values.dtype)
        try:
            self._run("ah_round", self.c.round, OL.TYPE_IDS[values.dtype], vp, vvp, off, values.size, ndigits, mode, m,
                      OL.load_oracle().pow10(abs(ndigits)), ob)
            st = STATUS_OK
        except ah.ErrOverflow:
            st = STATUS_EOVERFLOW
        return st, ob.download(values.dtype, values.size)

    def arithmetic_ext(self, op, shape, l, lvalid, loff, r, rvalid, roff, scalar_valid=True, *, misalign_l=0, misalign_r=0, out_phase=0):
        import arrow_go_amd as ah
        l = np.ascontiguousarray(l); r = None if r is None else np.ascontiguousarray(r)
        arr = r if shape == 2 else l
        lb, lp = (None, l) if shape == 2 else self._up(l, misalign_l)
        rb, rp = (None, r) if (shape == 1 or r is None) else self._up(r, misalign_r)
        lvb, lvp = self._upbits(lvalid)
        rvb, rvp = self._upbits(rvalid)
        ob = self._out("out", arr.nbytes, self._phase(out_phase, 0, arr.dtype.itemsize), fill=0xCD)
        st, msg = STATUS_OK, ""
        try:
            self._run("ah_arithmetic_ext", self.c.arithmetic_ext, OL.TYPE_IDS[arr.dtype], op, shape, lp, lvp, loff, rp, rvp, roff,
                      scalar_valid, ob, arr.size)
        except ah.ErrOverflow as e:
            st, msg = STATUS_EOVERFLOW, str(e)
        except ah.ErrInvalid as e:
            st, msg = STATUS_EINVALID, str(e)
        return st, ob.download(arr.dtype, arr.size), msg

    def comparison(self, cmpop, shape, l, r, out_init, out_bit_offset=0, misalign=0):
        l = np.ascontiguousarray(l); r = np.ascontiguousarray(r)
        arr = r if shape == 2 else l
        lb, lp = (None, l) if shape == 2 else self._up(l, misalign)
        rb, rp = (None, r) if shape == 1 else self._up(r, misalign)
        out_init = np.ascontiguousarray(out_init, dtype=np.uint8)
        ob = self._out("out_bits", out_init.size, init=out_init)
        self._run("ah_comparison", self.c.comparison, cmpop, shape, OL.TYPE_IDS[arr.dtype], lp, rp, ob, arr.size, out_bit_offset)
        return ob.download(np.uint8, out_init.size)

    def count_set_bits(self, bits, off, n):
        b, p = self._upbits(bits)
        return self.c.count_set_bits(p, off, n)

    def bitmap_op(self, op, l, loff, r, roff, out_init, ooff, n):
        lb, lp = self._upbits(l); rb, rp = self._upbits(r)
        out_init = np.ascontiguousarray(out_init, dtype=np.uint8)
        ob = self._out("out", out_init.size, init=out_init)
        self._run("ah_bitmap_op", self.c.bitmap_op, op, lp, loff, rp, roff, ob, ooff, n)
        return ob.download(np.uint8, out_init.size)

    def copy_bitmap(self, src, soff, n, out_init, doff, invert=False):
        sb, sp = self._upbits(src)
        out_init = np.ascontiguousarray(out_init, dtype=np.uint8)
        ob = self._out("dst", out_init.size, init=out_init)
        self._run("ah_copy_bitmap", self.c.copy_bitmap, sp, soff, n, ob, doff, invert)
        return ob.download(np.uint8, out_init.size)

    def set_bits_to(self, out_init, off, n, value):
        out_init = np.ascontiguousarray(out_init, dtype=np.uint8)
        ob = self._out("bits", out_init.size, init=out_init)
        self._run("ah_set_bits_to", self.c.set_bits_to, ob, off, n, value)
        return ob.download(np.uint8, out_init.size)

    def kleene(self, op, lvalid, ldata, loff, rvalid, rdata, roff, ovalid_init, odata_init, ooff, n):
        lvb, lvp = self._upbits(lvalid); ldb, ldp = self._upbits(ldata)
        rvb, rvp = self._upbits(rvalid); rdb, rdp = self._upbits(rdata)
        ovalid_init = np.ascontiguousarray(ovalid_init, dtype=np.uint8)
        odata_init = np.ascontiguousarray(odata_init, dtype=np.uint8)
        ovb = self._out("out_valid", ovalid_init.size, init=ovalid_init)
        odb = self._out("out_data", odata_init.size, init=odata_init)
        self._run("ah_kleene", self.c.kleene, op, lvp, ldp, loff, rvp, rdp, roff, ovb, odb, ooff, n)
        return ovb.download(np.uint8, ovalid_init.size), odb.download(np.uint8, odata_init.size)

    def filter_count(self, fdata, fvalid, foff, n, null_sel):
        fb, fp = self._upbits(fdata); vb, vp = self._upbits(fvalid)
        return self.c.filter_count(fp, vp, foff, n, null_sel)

    def filter(self, values, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid, misalign=0, *, out_phase=0):
        """misalign shifts the value input alone; out_phase places the value output of both entry points"""
        values = np.ascontiguousarray(values)
        w = values.dtype.itemsize
        vb, vp = self._up(values, misalign)
        vvb, vvp = self._upbits(vvalid)
        fb, fp = self._upbits(fdata); fvb, fvp = self._upbits(fvalid)
        n_out = self.c.filter_count(fp, fvp, foff, n, null_sel)
        ob = self._out("out_values", n_out * w, self._phase(out_phase, 0, w), fill=0xCD)  # the library must not rely on a pre-zeroed value buffer
        ovb = self._out("out_valid", (n_out + 7) // 8, fill=0xCD) if want_valid else None
        nulls = self._run("ah_filter_primitive", self.c.filter_primitive, w, vp, vvp, voff, fp, fvp, foff, n, null_sel, n_out, ob, ovb)
        out = ob.download(values.dtype, n_out)
        ov = ovb.download(np.uint8, (n_out + 7) // 8) if want_valid else None
        # every Filter of the suite also goes through the one-call entry (ah_filter_primitive_once: outputs sized for n rows, count and
        # null count through the mailbox) and must give the same rows, validity bits, count and null count
        ob1 = self._out("out_values", n * w, self._phase(out_phase, 0, w), fill=0xCD)
        ovb1 = self._out("out_valid", (n + 7) // 8, fill=0xCD) if want_valid else None
        k1, nulls1 = self._run("ah_filter_primitive_once", self.c.filter_primitive_once, w, vp, vvp, voff, fp, fvp, foff, n, null_sel, ob1, ovb1)
        assert k1 == n_out, ("filter_primitive_once: rows selected", k1, n_out)
        assert ob1.download(values.dtype, n_out).tobytes() == out.tobytes(), "filter_primitive_once: values"
        if want_valid:
            assert nulls1 == nulls, ("filter_primitive_once: null count", nulls1, nulls)
            bits = lambda b: np.unpackbits(b, bitorder="little")[:n_out]
            assert (bits(ovb1.download(np.uint8, (n_out + 7) // 8)) == bits(ov)).all(), "filter_primitive_once: validity"
        return out, ov, nulls

    def filter_to_indices(self, fdata, fvalid, foff, n, null_sel, want_valid, *, out_phase=0):
        fb, fp = self._upbits(fdata); fvb, fvp = self._upbits(fvalid)
        n_out = self.c.filter_count(fp, fvp, foff, n, null_sel)
        ob = self._out("out_idx", n_out * 4, self._phase(out_phase, 0, 4))
        ovb = self._out("out_valid", (n_out + 7) // 8) if want_valid else None
        nulls = self._run("ah_filter_to_indices", self.c.filter_to_indices, fp, fvp, foff, n, null_sel, n_out, ob, ovb)
        return ob.download(np.uint32, n_out), (ovb.download(np.uint8, (n_out + 7) // 8) if want_valid else None), nulls

    def take(self, values, vvalid, voff, idx, ivalid, ioff, bounds_check, want_valid, *, misalign_values=0, misalign_idx=0, out_phase=0):
        import arrow_go_amd as ah
        values = np.ascontiguousarray(values); idx = np.ascontiguousarray(idx)
        w = values.dtype.itemsize
        vb, vp = self._up(values, misalign_values); vvb, vvp = self._upbits(vvalid)
        ib, ip = self._up(idx, misalign_idx); ivb, ivp = self._upbits(ivalid)
        ob = self._out("out_values", idx.size * w, self._phase(out_phase, 0, w), fill=0xCD)
        ovb = self._out("out_valid", (idx.size + 7) // 8) if want_valid else None
        try:
            nulls = self._run("ah_take_primitive", self.c.take_primitive, w, vp, vvp, voff, values.size, idx.dtype.itemsize,
                              idx.dtype.kind == "i", ip, ivp, ioff, idx.size, bounds_check, ob, ovb)
        except ah.ErrIndex as e:
            msg = str(e)
            assert msg.endswith("out of bounds"), msg
            return STATUS_EINDEX, None, None, 0, int(msg.split()[0])
        out = ob.download(values.dtype, idx.size)
        ov = ovb.download(np.uint8, (idx.size + 7) // 8) if want_valid else None
        return STATUS_OK, out, ov, nulls, 0

    # -- the *_dev flavours: worst-case outputs, status words fetched after the fact
    def filter_dev(self, values, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid, misalign=0, *, out_phase=0):
        values = np.ascontiguousarray(values)
        w = values.dtype.itemsize
        vb, vp = self._up(values, misalign)
        vvb, vvp = self._upbits(vvalid)
        fb, fp = self._upbits(fdata); fvb, fvp = self._upbits(fvalid)
        ob = self._out("out_values", n * w, self._phase(out_phase, 0, w), fill=0xCD)
        ovb = self._out("out_valid", (n + 7) // 8, fill=0xCD) if want_valid else None
        st = self._out("status_dev", 16, fill=0xCD)
        self._run("ah_filter_primitive_dev", self.c.filter_primitive_dev, w, vp, vvp, voff, fp, fvp, foff, n, null_sel, ob, ovb, st)
        n_out, nulls = (int(v) for v in st.download(np.int64, 2))
        out = ob.download(values.dtype, n_out)
        ov = ovb.download(np.uint8, (n_out + 7) // 8) if want_valid else None
        return out, ov, nulls

    def take_dev(self, values, vvalid, voff, idx, ivalid, ioff, want_valid, *, misalign_values=0, misalign_idx=0, out_phase=0):
        """→ (values, validity bytes, null count, position of the first out-of-range index or None)"""
        values = np.ascontiguousarray(values); idx = np.ascontiguousarray(idx)
        w = values.dtype.itemsize
        vb, vp = self._up(values, misalign_values); vvb, vvp = self._upbits(vvalid)
        ib, ip = self._up(idx, misalign_idx); ivb, ivp = self._upbits(ivalid)
        ob = self._out("out_values", idx.size * w, self._phase(out_phase, 0, w), fill=0xCD)
        ovb = self._out("out_valid", (idx.size + 7) // 8) if want_valid else None
        st = self._out("status_dev", 16, fill=0xCD)
        self._run("ah_take_primitive_dev", self.c.take_primitive_dev, w, vp, vvp, voff, values.size, idx.dtype.itemsize, idx.dtype.kind == "i",
                  ip, ivp, ioff, idx.size, ob, ovb, st)
        bad, nulls = (int(v) for v in st.download(np.uint64, 2))
        out = ob.download(values.dtype, idx.size)
        ov = ovb.download(np.uint8, (idx.size + 7) // 8) if want_valid else None
        return out, ov, nulls, (None if bad == 2**64 - 1 else bad)

    def cumulative_sum(self, values, valid, off, start=None, skip_nulls=False, checked=False, misalign=0, *, misalign_in=None, out_phase=None):
        import arrow_go_amd as ah
        values = np.ascontiguousarray(values)
        n = values.size
        w = values.dtype.itemsize
        vb, vp = self._up(values, misalign if misalign_in is None else misalign_in); vvb, vvp = self._upbits(valid)
        # the library must write every row, including the zero payload of null rows
        ob = self._out("out_values", n * w, self._phase(out_phase, misalign, w), fill=0xCD)
        # prepareCumulativeOutput pre-fills the validity with ones; only bits [0, n) are the library's
        ovb = self._out("out_valid", (n + 7) // 8, fill=0xFF) if valid is not None else None
        sb = np.array([start], dtype=values.dtype).tobytes() if start is not None else None
        try:
            nulls = self._run("ah_cumulative_sum", self.c.cumulative_sum, OL.TYPE_IDS[values.dtype], vp, vvp, off, n, sb, skip_nulls, checked,
                              ob, ovb)
        except ah.ErrOverflow as e:
            assert "overflow" in str(e)
            return STATUS_EOVERFLOW, None, None, 0
        out = ob.download(values.dtype, n)
        ov = ovb.download(np.uint8, (n + 7) // 8) if ovb is not None else None
        return STATUS_OK, out, ov, nulls

    def cast_numeric(self, values, out_dtype, valid=None, off=0, allow_int_overflow=False, allow_float_truncate=False, misalign=0, *,
                     misalign_in=None, out_phase=None):
        import arrow_go_amd as ah
        values = np.ascontiguousarray(values)
        od = np.dtype(out_dtype)
        vb, vp = self._up(values, misalign if misalign_in is None else misalign_in); vvb, vvp = self._upbits(valid)
        ob = self._out("out_values", values.size * od.itemsize, self._phase(out_phase, misalign, od.itemsize), fill=0xCD)
        try:
            self._run("ah_cast_numeric", self.c.cast_numeric, OL.TYPE_IDS[values.dtype], OL.TYPE_IDS[od], vp, vvp, off, values.size,
                      allow_int_overflow, allow_float_truncate, ob)
        except ah.ErrInvalid as e:
            return STATUS_EINVALID, None, str(e)
        return STATUS_OK, ob.download(od, values.size), ""

    def shift_time(self, values, out_dtype, op, factor, check, valid=None, off=0, misalign=0, *, misalign_in=None, out_phase=None):
        import arrow_go_amd as ah
        values = np.ascontiguousarray(values)
        od = np.dtype(out_dtype)
        vb, vp = self._up(values, misalign if misalign_in is None else misalign_in); vvb, vvp = self._upbits(valid)
        ob = self._out("out_values", values.size * od.itemsize, self._phase(out_phase, misalign, od.itemsize), fill=0xCD)
        try:
            self._run("ah_shift_time", self.c.shift_time, values.dtype.itemsize * 8, od.itemsize * 8, op, factor, check, vp, vvp, off,
                      values.size, ob)
        except ah.ErrInvalid as e:
            return STATUS_EINVALID, None, e.bad_value
        return STATUS_OK, ob.download(od, values.size), 0

    def cast_bool_to_numeric(self, bits, off, n, out_dtype, *, out_phase=0):
        od = np.dtype(out_dtype)
        bb, bp = self._upbits(bits)
        ob = self._out("out_values", n * od.itemsize, self._phase(out_phase, 0, od.itemsize), fill=0xCD)
        self._run("ah_cast_bool_to_numeric", self.c.cast_bool_to_numeric, OL.TYPE_IDS[od], bp, off, n, ob)
        return ob.download(od, n)

    def is_in(self, values, valid, off, set_values, set_valid, set_off, null_behavior, out_off=0, fill=0, misalign=0):
        values = np.ascontiguousarray(values); set_values = np.ascontiguousarray(set_values)
        n = values.size
        vb, vp = self._up(values, misalign); vvb, vvp = self._upbits(valid)
        sb, sp = self._up(set_values) if set_values.size else (None, None); svb, svp = self._upbits(set_valid)
        nb = (out_off + n + 7) // 8 + 1
        odb = self._out("out_data", nb, fill=fill); ovb = self._out("out_valid", nb, fill=fill)
        self._run("ah_is_in", self.c.is_in, values.dtype.itemsize, vp, vvp, off, n, sp, svp, set_off, set_values.size, null_behavior, odb, ovb, out_off)
        return odb.download(np.uint8, nb), ovb.download(np.uint8, nb)

    def take_binary(self, offsets, data, vvalid, voff, nvalues, idx, ivalid, ioff, want_valid, *, misalign_offsets=0, misalign_data=0,
                    misalign_idx=0, out_phase=0, data_phase=0):
        """out_phase places the output offsets (a multiple of the offset width), data_phase the output bytes"""
        import arrow_go_amd as ah
        offsets = np.ascontiguousarray(offsets); idx = np.ascontiguousarray(idx)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        n = idx.size
        w = offsets.dtype.itemsize
        ofb, ofp = self._up(offsets, misalign_offsets); db, dp = self._up(data, misalign_data) if data.size else (None, None)
        vvb, vvp = self._upbits(vvalid); ib, ip = self._up(idx, misalign_idx) if n else (None, None); ivb, ivp = self._upbits(ivalid)
        oob = self._out("out_offsets", (n + 1) * w, self._phase(out_phase, 0, w), fill=0xCD)
        ovb = self._out("out_valid", (n + 7) // 8) if want_valid else None
        try:
            nulls, total = self._run("ah_take_binary_offsets", self.c.take_binary_offsets, w, ofp, vvp, voff, nvalues, idx.dtype.itemsize,
                                     idx.dtype.kind == "i", ip, ivp, ioff, n, oob, ovb)
        except ah.ErrIndex as e:
            return STATUS_EINDEX, None, None, None, 0, int(str(e).split()[0])
        odb = self._out("out_data", total, data_phase, fill=0xCD)
        self._run("ah_take_binary_data", self.c.take_binary_data, w, ofp, dp, voff, idx.dtype.itemsize, ip, n, oob, odb)
        return (STATUS_OK, oob.download(offsets.dtype, n + 1), odb.download(np.uint8, total),
                (ovb.download(np.uint8, (n + 7) // 8) if want_valid else None), nulls, 0)

    def filter_binary(self, offsets, data, vvalid, voff, fdata, fvalid, foff, n, null_sel, want_valid):
        """filter = GetTakeIndices + var-length take (ah_filter_count → ah_filter_to_indices → ah_take_binary_*)"""
        offsets = np.ascontiguousarray(offsets); data = np.ascontiguousarray(data, dtype=np.uint8)
        w = offsets.dtype.itemsize
        ofb, ofp = self._up(offsets); db, dp = self._up(data) if data.size else (None, None)
        vvb, vvp = self._upbits(vvalid); fb, fp = self._upbits(fdata); fvb, fvp = self._upbits(fvalid)
        n_out = self.c.filter_count(fp, fvp, foff, n, null_sel)
        ib = self._out("out_idx", n_out * 4); ivb = self._out("out_valid", (n_out + 7) // 8)
        idx_nulls = self._run("ah_filter_to_indices", self.c.filter_to_indices, fp, fvp, foff, n, null_sel, n_out, ib, ivb)
        oob = self._out("out_offsets", (n_out + 1) * w)
        ovb = self._out("out_valid", (n_out + 7) // 8) if want_valid else None
        nulls, total = self._run("ah_take_binary_offsets", self.c.take_binary_offsets, w, ofp, vvp, voff, n, 4, False, ib,
                                 ivb if idx_nulls else None, 0, n_out, oob, ovb)
        odb = self._out("out_data", total)
        self._run("ah_take_binary_data", self.c.take_binary_data, w, ofp, dp, voff, 4, ib, n_out, oob, odb)
        return (oob.download(offsets.dtype, n_out + 1), odb.download(np.uint8, total),
                (ovb.download(np.uint8, (n_out + 7) // 8) if want_valid else None), nulls)

    def sort_indices_multi(self, columns, *, out_phase=0):
        keep, keys = [], []
        n = np.asarray(columns[0][0]).size
        for values, valid, off, desc, nfirst in columns:
            values = np.ascontiguousarray(values)
            vb, vp = self._up(values); vvb, vvp = self._upbits(valid)
            keep += [vb, vvb]
            keys.append((OL.TYPE_IDS[values.dtype], vp, vvp, off, desc, nfirst))
        ob = self._out("out_indices", n * 8, self._phase(out_phase, 0, 8))
        self._run("ah_sort_indices_multi", self.c.sort_indices_multi, keys, n, ob)
        return ob.download(np.uint64, n)

    def min_max(self, values, misalign=0):
        values = np.ascontiguousarray(values)
        vb, vp = self._up(values, misalign) if values.size else (None, None)
        return self.c.min_max(OL.TYPE_IDS[values.dtype], vp, values.size, values.dtype)

    def sort_indices(self, values, valid, off, descending=False, nulls_at_start=False, misalign=0, *, out_phase=0):
        """misalign shifts the value input alone; out_phase (0 or 8) places the indices"""
        values = np.ascontiguousarray(values)
        n = values.size
        vb, vp = self._up(values, misalign); vvb, vvp = self._upbits(valid)
        ob = self._out("out_indices", n * 8, self._phase(out_phase, 0, 8), fill=0xCD)
        self._run("ah_sort_indices", self.c.sort_indices, OL.TYPE_IDS[values.dtype], vp, vvp, off, n, descending, nulls_at_start, ob)
        return ob.download(np.uint64, n)

    def hash_encode(self, keys, valid, off, encode_nulls, *, misalign_keys=0, out_phase=0, dict_phase=0):
        """out_phase places the ids (a multiple of 4), dict_phase the dictionary (0 or 8)"""
        keys = np.ascontiguousarray(keys).view(np.uint64)
        n = keys.size
        kb, kp = self._up(keys, misalign_keys); vb, vp = self._upbits(valid)
        idb = self._out("out_ids", n * 4, self._phase(out_phase, 0, 4)); idvb = self._out("out_ids_valid", (n + 7) // 8)
        db = self._out("out_dict", (n + 1) * 8, self._phase(dict_phase, 0, 8))
        nd, nid = self._run("ah_hash_u64_encode", self.c.hash_u64_encode, kp, vp, off, n, encode_nulls, idb, idvb, db)
        return idb.download(np.int32, n), idvb.download(np.uint8, (n + 7) // 8), db.download(np.uint64, nd), nid

    def hash_binary_encode(self, offsets, data, valid, off, n, encode_nulls):
        offsets = np.ascontiguousarray(offsets); data = np.ascontiguousarray(data, dtype=np.uint8)
        ofb, ofp = self._up(offsets); db, dp = self._up(data) if data.size else (None, None); vb, vp = self._upbits(valid)
        idb = self._out("out_ids", n * 4); idvb = self._out("out_ids_valid", (n + 7) // 8); frb = self._out("out_first_rows", (n + 1) * 8)
        nd, nid = self._run("ah_hash_binary_encode", self.c.hash_binary_encode, offsets.dtype.itemsize, ofp, dp, vp, off, n, encode_nulls,
                            idb, idvb, frb)
        return idb.download(np.int32, n), idvb.download(np.uint8, (n + 7) // 8), frb.download(np.int64, nd), nid

    def hash_fixed_encode(self, data, w, valid, off, n, encode_nulls):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        db, dp = self._up(data); vb, vp = self._upbits(valid)
        idb = self._out("out_ids", n * 4); idvb = self._out("out_ids_valid", (n + 7) // 8); frb = self._out("out_first_rows", (n + 1) * 8)
        dcb = self._out("out_dict", (n + 1) * w)
        nd, nid = self._run("ah_hash_fixed_encode", self.c.hash_fixed_encode, w, dp, vp, off, n, encode_nulls, idb, idvb, frb, dcb)
        return idb.download(np.int32, n), idvb.download(np.uint8, (n + 7) // 8), frb.download(np.int64, nd), nid, dcb.download(np.uint8, nd * w)

    def hash_sum(self, kind, keys, kvalid, koff, vals, vvalid, voff):
        keys = np.ascontiguousarray(keys).view(np.uint64); vals = np.ascontiguousarray(vals)
        n = keys.size
        kb, kp = self._up(keys); kvb, kvp = self._upbits(kvalid)
        xb, xp = self._up(vals); xvb, xvp = self._upbits(vvalid)
        okb = self._out("out_keys", (n + 1) * 8); osb = self._out("out_sums", (n + 1) * 8); ocb = self._out("out_counts", (n + 1) * 8)
        ofb = self._out("out_first_rows", (n + 1) * 8)
        ng, nid = self._run("ah_hash_sum_" + kind, self.c.hash_sum, kind, kp, kvp, koff, xp, xvp, voff, n, okb, osb, ocb, ofb)
        return okb.download(np.uint64, ng), osb.download(vals.dtype, ng), ocb.download(np.int64, ng), nid, ofb.download(np.int64, ng)

    def copy(self, src, *, src_phase=0, dst_phase=0):
        """ah_copy_async of the bytes `src` between two device ranges at the given byte phases → the destination's bytes"""
        from arrow_go_amd._native import lib, check
        src = np.ascontiguousarray(src, dtype=np.uint8)
        sb, sp = self._up(src, src_phase)
        ob = self._out("dst", src.size, dst_phase, fill=0xCD)
        self._run("ah_copy_async", lambda: check(self.c.handle, lib.ah_copy_async(self.c.handle, ob.ptr, sp, src.size)))
        return ob.download(np.uint8, src.size)

    def cmp_filter_sum_i64(self, cmpop, x, valid, off, thr, misalign=0):
        x = np.ascontiguousarray(x)
        xb, xp = self._up(x, misalign); vb, vp = self._upbits(valid)
        return self.c.cmp_filter_sum_i64(cmpop, xp, vp, off, x.size, int(thr))

    def cmp_filter_sum_f64(self, cmpop, x, valid, off, thr, misalign=0):
        x = np.ascontiguousarray(x)
        xb, xp = self._up(x, misalign); vb, vp = self._upbits(valid)
        return self.c.cmp_filter_sum_f64(cmpop, xp, vp, off, x.size, float(thr))
