"""Host model of the six entry points of ah_conditional.hip, byte for byte (plain numpy; pinned against pyarrow in
tests/test_conditional_model_host.py).

Semantics (Arrow C++'s): if_else(cond, l, r) is null where cond is null, otherwise l[i] or r[i] with that side's validity; a
directed fill gives a null row the nearest valid row before (forward) / after (backward) it and leaves it null when there is none.
Where Arrow leaves bytes unspecified the library does not, and the model states the rule: the payload under a null slot of a
fixed-width output is zero bytes, a null data bit is 0, a null var-length row has length 0, the unused bits of a bitmap's last
byte are 0, output bitmaps and offsets start at 0.

Buffers are numpy uint8 arrays (offsets: int32 / int64 arrays), bitmaps LSB-first.  A side is a tuple laid out like ah_cond_side:
    (offset_width, byte_width, offsets, data, valid, off, broadcast)
offset_width 0: fixed slots of byte_width bytes, row i at data[(off + i) * byte_width:]; for the Boolean call `data` is a bitmap
read at bit off + i; offset_width 4 / 8: row i is data[offsets[off + i]:offsets[off + i + 1]].  valid: a bitmap read at bit
off + i, or None.  broadcast: every row reads element off."""
import numpy as np


def bits(bitmap, off, n, broadcast=False):
    """rows → bool array of n: bit off + i of the bitmap (None: all ones); broadcast: bit off for every row"""
    if bitmap is None:
        return np.ones(n, bool)
    if broadcast:
        return np.full(n, bool((int(bitmap[off >> 3]) >> (off & 7)) & 1))
    return np.unpackbits(np.asarray(bitmap, np.uint8), bitorder="little")[off:off + n].astype(bool)


def pack(flags):
    """bool array → bitmap from bit 0: ceil(n / 8) bytes, the unused bits 0"""
    return np.packbits(np.asarray(flags, bool), bitorder="little")


def _pick(cond_data, cond_valid, cond_off, left, right, n):
    """→ (take_left, take_right): bool arrays; a row in neither is null"""
    cv, cd = bits(cond_valid, cond_off, n), bits(cond_data, cond_off, n)
    lv, rv = bits(left[4], left[5], n, left[6]), bits(right[4], right[5], n, right[6])
    return cv & cd & lv, cv & ~cd & rv


def _has_validity(cond_valid, left, right):
    return cond_valid is not None or left[4] is not None or right[4] is not None


def _fixed_rows(side, n):
    _, w, _, data, _, off, broadcast = side
    data = np.asarray(data, np.uint8)
    if broadcast:
        return np.broadcast_to(data[off * w:(off + 1) * w], (n, w))
    return data[off * w:(off + n) * w].reshape(n, w)


def if_else(cond_data, cond_valid, cond_off, left, right, n):
    """ah_if_else → (out_values: n * byte_width bytes, out_valid: ceil(n / 8) bytes or None when no input has a bitmap)"""
    w = left[1]
    assert w == right[1]
    tl, tr = _pick(cond_data, cond_valid, cond_off, left, right, n)
    out = np.zeros((n, w), np.uint8)
    out[tl] = _fixed_rows(left, n)[tl]
    out[tr] = _fixed_rows(right, n)[tr]
    return out.reshape(-1), (pack(tl | tr) if _has_validity(cond_valid, left, right) else None)


def if_else_boolean(cond_data, cond_valid, cond_off, left, right, n):
    """ah_if_else_boolean → (out_data, out_valid or None): bitmaps from bit 0; a null row's data bit is 0"""
    tl, tr = _pick(cond_data, cond_valid, cond_off, left, right, n)
    ld, rd = bits(left[3], left[5], n, left[6]), bits(right[3], right[5], n, right[6])
    return pack((tl & ld) | (tr & rd)), (pack(tl | tr) if _has_validity(cond_valid, left, right) else None)


def _var_rows(side, n):
    """→ (start, length) int64 arrays of the side's n rows"""
    ow, _, offsets, _, _, off, broadcast = side
    o = np.asarray(offsets).astype(np.int64)
    if broadcast:
        return np.full(n, o[off]), np.full(n, o[off + 1] - o[off])
    return o[off:off + n], o[off + 1:off + n + 1] - o[off:off + n]


class OffsetOverflow(Exception):
    """the bytes do not fit 4-byte offsets: the library's AH_EINVALID "binary output offset overflow\""""


def if_else_binary_offsets(cond_data, cond_valid, cond_off, left, right, n, out_offset_width):
    """ah_if_else_binary_offsets → (out_offsets[n + 1], out_valid or None, total bytes)"""
    tl, tr = _pick(cond_data, cond_valid, cond_off, left, right, n)
    lens = np.where(tl, _var_rows(left, n)[1], 0) + np.where(tr, _var_rows(right, n)[1], 0)
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    if out_offset_width == 4 and n and offs[-1] > 2**31 - 1:
        raise OffsetOverflow(int(offs[-1]))
    out = offs.astype(np.int32 if out_offset_width == 4 else np.int64)
    return out, (pack(tl | tr) if _has_validity(cond_valid, left, right) else None), int(offs[-1])


def if_else_binary_data(cond_data, cond_valid, cond_off, left, right, n, out_offsets):
    """ah_if_else_binary_data → the bytes (out_offsets[n] of them)"""
    tl, tr = _pick(cond_data, cond_valid, cond_off, left, right, n)
    out = np.zeros(int(out_offsets[n]) if n else 0, np.uint8)
    for take, side in ((tl, left), (tr, right)):
        start, length = _var_rows(side, n)
        data = np.asarray(side[3], np.uint8)
        for i in np.flatnonzero(take & (length > 0)):
            out[out_offsets[i]:out_offsets[i + 1]] = data[start[i]:start[i] + length[i]]
    return out


def fill_sources(valid, off, n, direction):
    """→ (source row of every row as int64, −1 where there is none)"""
    v = bits(valid, off, n)
    rows = np.arange(n, dtype=np.int64)
    if direction == 0:
        return np.maximum.accumulate(np.where(v, rows, -1)) if n else rows
    big = np.int64(2**62)
    src = np.minimum.accumulate(np.where(v, rows, big)[::-1])[::-1] if n else rows
    return np.where(src == big, -1, src)


def fill_null_indices(valid, off, n, direction):
    """ah_fill_null_indices → (out_idx uint32 — 0 where there is no source —, out_idx_valid bitmap, null count)"""
    src = fill_sources(valid, off, n, direction)
    ok = src >= 0
    return np.where(ok, src, 0).astype(np.uint32), pack(ok), int(n - ok.sum())


def fill_null_directed(byte_width, values, valid, off, n, direction):
    """ah_fill_null_directed → (out_values: n * byte_width bytes — zero where there is no source —, out_valid bitmap, null count);
    `values` is the buffer from its element 0, row i is element off + i"""
    src = fill_sources(valid, off, n, direction)
    ok = src >= 0
    rows = np.asarray(values, np.uint8)[off * byte_width:(off + n) * byte_width].reshape(n, byte_width)
    out = np.zeros((n, byte_width), np.uint8)
    out[ok] = rows[src[ok]]
    return out.reshape(-1), pack(ok), int(n - ok.sum())
