"""A model of the LZ4 block and frame formats in plain Python (lz4_Block_format.md, lz4_Frame_format.md), for the tests of the device
decoder (csrc/ah_lz4.h) and the frame planner (host/lz4_frame.h): xxh32, a frame assembler that takes a block list, flags and a BD
code, a small greedy block compressor, and a sequential block decoder.  Depends on nothing beyond numpy and pyarrow; pyarrow's codec
(liblz4) is the independent implementation the model is pinned to in tests/test_lz4_host.py."""
import struct

MAGIC = 0x184D2204
BLOCK_MAX = 65536
FLG_VERSION, FLG_INDEP, FLG_BLOCK_CHECKSUM, FLG_CONTENT_SIZE, FLG_CONTENT_CHECKSUM, FLG_RESERVED, FLG_DICT_ID = 0x40, 0x20, 0x10, 0x08, 0x04, 0x02, 0x01
M32 = 0xFFFFFFFF


# ---- xxh32 ------------------------------------------------------------------------------------------------------------------------
def xxh32(data, seed=0):
    P1, P2, P3, P4, P5 = 2654435761, 2246822519, 3266489917, 668265263, 374761393
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & M32
    data = bytes(data)
    n, p = len(data), 0
    if n >= 16:
        v = [(seed + P1 + P2) & M32, (seed + P2) & M32, seed & M32, (seed - P1) & M32]
        while p + 16 <= n:
            for k in range(4):
                v[k] = (rotl((v[k] + struct.unpack_from("<I", data, p + 4 * k)[0] * P2) & M32, 13) * P1) & M32
            p += 16
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) + rotl(v[3], 18)) & M32
    else:
        h = (seed + P5) & M32
    h = (h + n) & M32
    while p + 4 <= n:
        h = (rotl((h + struct.unpack_from("<I", data, p)[0] * P3) & M32, 17) * P4) & M32
        p += 4
    while p < n:
        h = (rotl((h + data[p] * P5) & M32, 11) * P1) & M32
        p += 1
    h ^= h >> 15
    h = (h * P2) & M32
    h ^= h >> 13
    h = (h * P3) & M32
    h ^= h >> 16
    return h


# ---- blocks -----------------------------------------------------------------------------------------------------------------------
def _length_bytes(n):
    """the extension bytes of a length whose nibble is 15: n = the part beyond 15"""
    out = bytearray()
    while n >= 255:
        out.append(255)
        n -= 255
    out.append(n)
    return bytes(out)


def sequence(literals, offset=None, match_len=None):
    """one sequence: literals, then (unless it is the block's last) a match of match_len >= 4 bytes `offset` back"""
    literals = bytes(literals)
    ll = len(literals)
    ml = 0 if offset is None else match_len - 4
    out = bytearray([(min(ll, 15) << 4) | min(ml, 15)])
    if ll >= 15:
        out += _length_bytes(ll - 15)
    out += literals
    if offset is not None:
        out += struct.pack("<H", offset)
        if ml >= 15:
            out += _length_bytes(ml - 15)
    return bytes(out)


def compress_block(data):
    """a greedy compressor: the most recent earlier occurrence of the next four bytes, extended as far as it goes.  Keeps the
    encoder's end-of-block rules (the last five bytes are literals, no match starts in the last twelve), so liblz4 takes its blocks."""
    data = bytes(data)
    n = len(data)
    out = bytearray()
    table = {}
    anchor = i = 0
    limit = n - 12          # a match starts before this position …
    match_end = n - 5       # … and ends at or before this one
    while i < limit:
        key = data[i:i + 4]
        cand = table.get(key)
        table[key] = i
        if cand is None or i - cand > 65535:
            i += 1
            continue
        m = 4
        while i + m < match_end and data[cand + m] == data[i + m]:
            m += 1
        out += sequence(data[anchor:i], i - cand, m)
        i += m
        anchor = i
    out += sequence(data[anchor:])
    return bytes(out)


def decode_block(src, dst_len):
    """the block's dst_len bytes, or None if the block is corrupt or produces another length.  The rules of the device decoder: every
    read inside src, every write inside dst_len, 1 <= offset <= bytes produced; the encoder's end-of-block rules are not enforced."""
    src = bytes(src)
    n, sp = len(src), 0
    out = bytearray()
    while True:
        if sp >= n:
            return None
        token = src[sp]
        sp += 1
        ll = token >> 4
        if ll == 15:
            while True:
                if sp >= n:
                    return None
                b = src[sp]
                sp += 1
                ll += b
                if b != 255:
                    break
        if ll > n - sp or ll > dst_len - len(out):
            return None
        out += src[sp:sp + ll]
        sp += ll
        if sp == n:
            break
        if n - sp < 2:
            return None
        offset = src[sp] | (src[sp + 1] << 8)
        sp += 2
        if offset == 0 or offset > len(out):
            return None
        ml = token & 15
        if ml == 15:
            while True:
                if sp >= n:
                    return None
                b = src[sp]
                sp += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        if ml > dst_len - len(out):
            return None
        start = len(out) - offset
        if offset >= ml:
            out += out[start:start + ml]
        else:
            for k in range(ml):
                out.append(out[start + k])
    return bytes(out) if len(out) == dst_len else None


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def frame(blocks, flg=FLG_VERSION | FLG_INDEP, bd_code=4, content_size=None, dict_id=None, content=None, header_checksum=None,
          trailing=b""):
    """blocks: [(bytes, stored)].  The flags decide which optional fields are written: content_size with FLG_CONTENT_SIZE, dict_id
    with FLG_DICT_ID, a checksum per block with FLG_BLOCK_CHECKSUM, xxh32(content) behind the EndMark with FLG_CONTENT_CHECKSUM."""
    desc = bytearray([flg, (bd_code & 7) << 4])
    if flg & FLG_CONTENT_SIZE:
        desc += struct.pack("<Q", content_size)
    if flg & FLG_DICT_ID:
        desc += struct.pack("<I", dict_id)
    hc = (xxh32(desc) >> 8) & 0xFF if header_checksum is None else header_checksum
    out = bytearray(struct.pack("<I", MAGIC)) + desc + bytes([hc])
    for data, stored in blocks:
        out += struct.pack("<I", len(data) | (0x80000000 if stored else 0)) + bytes(data)
        if flg & FLG_BLOCK_CHECKSUM:
            out += struct.pack("<I", xxh32(data))
    out += struct.pack("<I", 0)
    if flg & FLG_CONTENT_CHECKSUM:
        out += struct.pack("<I", xxh32(content))
    return bytes(out) + trailing


def split_blocks(data, compress=compress_block, block=BLOCK_MAX):
    """data cut into `block`-byte pieces, each compressed on its own — stored where that is not smaller"""
    data = bytes(data)
    out = []
    for at in range(0, len(data), block):
        piece = data[at:at + block]
        c = compress(piece)
        out.append((c, False) if len(c) < len(piece) else (piece, True))
    return out


def independent_frame(data, compress=compress_block, **kw):
    return frame(split_blocks(data, compress), **kw)


def parse_frame(buf):
    """(flg, bd, [(bytes, stored)], end) of a frame without optional header fields and block checksums — what the helpers here and
    pyarrow's codec write"""
    flg, bd = buf[4], buf[5]
    at = 7 + (8 if flg & FLG_CONTENT_SIZE else 0) + (4 if flg & FLG_DICT_ID else 0)
    blocks = []
    while True:
        w = struct.unpack_from("<I", buf, at)[0]
        at += 4
        if w == 0:
            break
        size = w & 0x7FFFFFFF
        blocks.append((bytes(buf[at:at + size]), bool(w >> 31)))
        at += size
    return flg, bd, blocks, at
