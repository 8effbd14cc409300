"""Re-frames the buffers of an LZ4-compressed Arrow IPC stream, for tests/test_ipc_lz4_device.py: pyarrow (Arrow C++) writes frames of
LINKED blocks for every buffer beyond one block, the reference's writer frames of independent ones — so a pyarrow stream is taken
apart message by message, every buffer's frame is replaced, and the metadata is patched in place: the Buffer {offset, length} structs
and Message.bodyLength are fixed-size int64 fields, reached through three vtable hops from the root (flatbuffers internals: a table
starts with an int32 back to its vtable, the vtable is [u16 bytes, u16 table bytes, u16 offset of field 0, …]).  No flatbuffers module
is needed."""
import struct

import pyarrow as pa

from tests import lz4_model as M

HEADER_DICTIONARY_BATCH, HEADER_RECORD_BATCH = 2, 3


def _field(meta, table, index):
    """position of field `index` of the table at `table`, or 0"""
    vt = table - struct.unpack_from("<i", meta, table)[0]
    vt_len = struct.unpack_from("<H", meta, vt)[0]
    slot = 4 + 2 * index
    if slot + 2 > vt_len:
        return 0
    off = struct.unpack_from("<H", meta, vt + slot)[0]
    return table + off if off else 0


def _indirect(meta, table, index):
    f = _field(meta, table, index)
    return f + struct.unpack_from("<I", meta, f)[0] if f else 0


def raw_block(data):
    """one block by liblz4's block compressor (pyarrow's "lz4_raw" codec)"""
    return pa.Codec("lz4_raw").compress(data).to_pybytes()


def independent(plain, index, stored):
    """the default replacement: a frame of independent 64 KiB blocks, whatever the buffer was (a stored buffer stays stored)"""
    return None if stored else M.independent_frame(plain, compress=raw_block)


def rewrite(stream, reframe=independent):
    """stream: bytes of an IPC stream written with compression="lz4".  reframe(plain bytes, running buffer index, was stored) → the
    frame to put in the buffer's place, or None to keep the buffer's bytes.  Returns the new stream."""
    stream = bytes(stream)
    out = bytearray()
    at, index = 0, 0
    while at < len(stream):
        word = struct.unpack_from("<I", stream, at)[0]
        assert word == 0xFFFFFFFF, "pre-0.15 framing is not handled"
        mlen = struct.unpack_from("<i", stream, at + 4)[0]
        if mlen == 0:
            out += stream[at:at + 8]
            at += 8
            break
        meta = bytearray(stream[at + 8:at + 8 + mlen])
        msg = struct.unpack_from("<I", meta, 0)[0]
        kind = meta[_field(meta, msg, 1)] if _field(meta, msg, 1) else 0
        blen_at = _field(meta, msg, 3)
        blen = struct.unpack_from("<q", meta, blen_at)[0] if blen_at else 0
        body = stream[at + 8 + mlen:at + 8 + mlen + blen]
        at += 8 + mlen + blen
        rb = 0
        if kind == HEADER_RECORD_BATCH:
            rb = _indirect(meta, msg, 2)
        elif kind == HEADER_DICTIONARY_BATCH:
            rb = _indirect(meta, _indirect(meta, msg, 2), 1)
        if rb and _field(meta, rb, 3) and blen:
            bufs = _indirect(meta, rb, 2)
            nbufs = struct.unpack_from("<I", meta, bufs)[0]
            new_body = bytearray()
            for i in range(nbufs):
                e = bufs + 4 + 16 * i
                off, ln = struct.unpack_from("<qq", meta, e)
                piece = body[off:off + ln]
                if ln >= 8:
                    ulen = struct.unpack_from("<q", piece, 0)[0]
                    stored = ulen == -1
                    plain = piece[8:] if stored else pa.Codec("lz4").decompress(piece[8:], decompressed_size=ulen).to_pybytes()
                    f = reframe(plain, index, stored)
                    index += 1
                    if f is not None:
                        piece = struct.pack("<q", len(plain)) + f
                struct.pack_into("<qq", meta, e, len(new_body), len(piece))
                new_body += piece + bytes(-len(piece) % 8)
            struct.pack_into("<q", meta, blen_at, len(new_body))
            body = bytes(new_body)
        out += struct.pack("<Ii", 0xFFFFFFFF, mlen) + meta + body
    return bytes(out) + stream[at:]
