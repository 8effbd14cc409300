"""The IPC writer: ah_lz4_compress_blocks against the host harness of tests/test_lz4_enc_host.py — the same header
compiled for the host, lanes in a loop — byte for byte, ah_ipc_pack_body against the bytes it is asked to put together, and
Session.write_ipc against pyarrow's reader and this project's own."""
import shutil
import struct
import tempfile

import numpy as np
import pyarrow as pa
import pytest

import arrow_go_amd as ah
from tests import lz4_enc_vectors as EV
from tests import lz4_model as M
from tests.test_lz4_enc_host import build_harness, compress_lines, compressed

pytestmark = pytest.mark.gpu
GUARD = 64


# ---- the C ABI: the block compressor -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness_answers():
    """every vector through the host harness: [(stored, lz4 size, bytes)]"""
    d = tempfile.mkdtemp(prefix="lz4_enc_harness_")
    try:
        run = build_harness(d)
        return [compressed(a) for a in run(compress_lines([data for _, data in EV.vectors()]))]
    finally:
        shutil.rmtree(d, ignore_errors=True)


def run_compress(ctx, datas, src_mis=0, dst_mis=0):
    """the blocks back to back (each at src_mis past a multiple of 16), their slots with GUARD bytes of 0xA5 between them, one
    launch → ([(stored, bytes written)], guards intact)"""
    src, table, dst_at = bytearray(), [], GUARD + dst_mis
    for data in datas:
        src += b"\x5a" * ((-len(src)) % 16 + src_mis)
        table.append((len(src), len(data), dst_at))
        src += data
        dst_at += len(data) + GUARD
        dst_at += (-dst_at) % 16 + dst_mis
    dsrc = ctx.to_device(np.frombuffer(bytes(src) + b"\x5a", np.uint8), pad=16)
    ddst = ctx.alloc(dst_at + 16)
    ddst.memset(0xA5)
    sizes, stored = ctx.lz4_compress_blocks(dsrc, len(src), ddst, dst_at, table)
    host = ddst.download(np.uint8, dst_at).tobytes()
    outs, guards_ok, prev_end = [], True, 0
    for (_, _, d0), size, st in zip(table, sizes, stored):
        guards_ok &= host[prev_end:d0] == b"\xa5" * (d0 - prev_end)
        outs.append((bool(st), host[d0:d0 + size]))
        prev_end = d0 + int(size)
    guards_ok &= host[prev_end:] == b"\xa5" * (dst_at - prev_end)
    dsrc.free()
    ddst.free()
    return outs, guards_ok


@pytest.mark.parametrize("src_mis,dst_mis", [(0, 0), (5, 0), (3, 11)])
def test_device_bytes_are_the_harness_bytes(ctx, harness_answers, src_mis, dst_mis):
    """all vectors in one launch; what lies behind a block's bytes in its slot, and between the slots, is untouched"""
    vecs = EV.vectors()
    outs, guards_ok = run_compress(ctx, [data for _, data in vecs], src_mis, dst_mis)
    assert guards_ok
    for (name, data), (stored, out), (h_stored, h_size, h_out) in zip(vecs, outs, harness_answers):
        assert stored == h_stored and out == h_out, name
        assert out == data if stored else M.decode_block(out, len(data)) == data, name


def test_compress_is_repeatable(ctx):
    """the table slot several lanes publish to in one step goes to the highest position by rule, not by what the hardware does:
    content with few distinct hashes, many blocks at once, twice"""
    rng = np.random.default_rng(3)
    datas = [rng.integers(0, 2 + k % 3, 65536 - 17 * k, dtype=np.uint8).tobytes() for k in range(24)]
    first, ok1 = run_compress(ctx, datas)
    second, ok2 = run_compress(ctx, datas, 7, 9)
    assert ok1 and ok2 and first == second
    assert all(not stored and M.decode_block(out, len(d)) == d for d, (stored, out) in zip(datas, first))


def test_compress_table_is_validated_before_the_launch(ctx):
    src, dst = ctx.to_device(np.zeros(256, np.uint8)), ctx.alloc(1 << 17)
    dst.memset(0xA5)
    for table in ([(0, 100, 0), (100, 100, 99)],            # overlapping slots
                  [(0, 100, 50), (100, 100, 0)],            # … descending ones
                  [(0, 100, (1 << 17) - 99)],               # a slot shorter than its block: the output ends inside it
                  [(0, 257, 0)], [(250, 10, 0)], [(-1, 10, 0)], [(0, 10, -1)], [(0, -1, 0)], [(0, 10, (1 << 17) + 1)],   # ranges outside the buffers
                  [(0, 65537, 0)]):
        with pytest.raises(ah.ErrInvalid):
            ctx.lz4_compress_blocks(src, 256 if table[0][1] <= 65536 else 1 << 17, dst, 1 << 17, table)
    assert dst.download(np.uint8, 1 << 17).tobytes() == b"\xa5" * (1 << 17)      # nothing was launched
    sizes, stored = ctx.lz4_compress_blocks(src, 256, dst, 1 << 17, [])
    assert len(sizes) == 0 and len(stored) == 0
    sizes, stored = ctx.lz4_compress_blocks(src, 256, dst, 1 << 17, [(0, 0, 0), (0, 256, 0)])   # an empty block takes no room
    assert list(sizes[:1]) == [0] and list(stored) == [1, 0]
    src.free()
    dst.free()


# ---- the C ABI: the body packer ------------------------------------------------------------------------------------------------------
def signed64(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def test_pack_body_puts_the_pieces_together(ctx):
    """pieces from all three sources at every mutual alignment of source and destination, with and without a size word in front,
    of lengths around the 16-byte line and the 256 lanes' reach"""
    rng = np.random.default_rng(8)
    comp = rng.integers(0, 256, 200000, dtype=np.uint8)
    plain = rng.integers(0, 256, 150001, dtype=np.uint8)
    lits = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    sources = (comp.tobytes(), plain.tobytes(), lits)
    rows, want, at = [], bytearray(), 0
    lengths = [0, 1, 3, 15, 16, 17, 31, 33, 255, 256, 257, 4095, 4099, 65536, 70001]
    for i in range(120):
        kind = i % 3
        n = min(lengths[(i * 7) % len(lengths)], 40 if kind == 2 else 1 << 20)
        src_off = int(rng.integers(0, len(sources[kind]) - n + 1))
        if i % 4 == 1:
            word = int(rng.integers(0, 1 << 32))
            rows.append((src_off, n, at + 4, signed64(kind | 0x100 | (word << 32))))
            want += struct.pack("<I", word)
            at += 4
        else:
            rows.append((src_off, n, at, kind))
        want += sources[kind][src_off:src_off + n]
        at += n
    # the last bytes of a source, misaligned: the line that cannot be read as whole words from inside the buffer
    for kind in (0, 1):
        rows.append((len(sources[kind]) - 37, 37, at, kind))
        want += sources[kind][-37:]
        at += 37
    dcomp, dplain = ctx.to_device(comp), ctx.to_device(plain)
    dst = ctx.alloc(at + GUARD)
    dst.memset(0xA5)
    ctx.ipc_pack_body(dcomp, len(comp), dplain, len(plain), lits, rows, dst, at)
    got = dst.download(np.uint8, at + GUARD).tobytes()
    assert got[:at] == bytes(want) and got[at:] == b"\xa5" * GUARD
    # rows that do not tile the output, or leave their source, are refused before anything runs
    dst.memset(0xA5)
    for bad, nbytes in (([(0, 10, 0, 0), (0, 10, 11, 0)], 21), ([(0, 10, 0, 0), (0, 10, 9, 0)], 19), ([(0, 10, 0, 0)], 11), ([(0, 10, 4, 0)], 14),
                        ([(0, 10, 0, 0x100)], 10), ([(len(comp) - 5, 10, 0, 0)], 10), ([(0, 301, 0, 2)], 301), ([(0, 10, 0, 3)], 10), ([(0, 10, 0, 4)], 10),
                        ([(-1, 10, 0, 0)], 10), ([(0, -1, 0, 0)], 0)):
        with pytest.raises(ah.ErrInvalid):
            ctx.ipc_pack_body(dcomp, len(comp), dplain, len(plain), lits, bad, dst, nbytes)
    assert dst.download(np.uint8, 64).tobytes() == b"\xa5" * 64
    ctx.ipc_pack_body(dcomp, len(comp), dplain, len(plain), lits, [], dst, 0)
    for b in (dcomp, dplain, dst):
        b.free()


# ---- the writer ----------------------------------------------------------------------------------------------------------------------
from arrow_go_amd import compute as ac      # noqa: E402
from tests import ipc_rewrite as R          # noqa: E402
from tests.test_ipc import TYPES, random_column   # noqa: E402

TEMPORAL = [pa.date32(), pa.date64(), pa.time32("s"), pa.time32("ms"), pa.time64("us"), pa.time64("ns"), pa.timestamp("s"),
            pa.timestamp("us", tz="UTC"), pa.timestamp("ns", tz="Europe/Paris"), pa.duration("ms")]
ROWS = [0, 1, 63, 64, 65, 1000, 70001]


@pytest.fixture(scope="module")
def sess():
    s = ac.Session(0)
    s.set_option("ipc_device_lz4_min_bytes", 0)    # every LZ4 body goes the device way when it is read back: the path is under test
    yield s
    s.close()


def temporal_column(rng, typ, n, p_null):
    storage = pa.int32() if typ.bit_width == 32 else pa.int64()
    mask = rng.random(n) < p_null if p_null else None
    return pa.array(rng.integers(0, 80000, n), mask=mask, type=storage).view(typ)


def dictionary_column(rng, index_type, values, n, p_null):
    mask = rng.random(n) < p_null if p_null else None
    return pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, len(values), n), mask=mask, type=index_type), values)


def all_types_table(n, seed=0):
    """every type in scope, once without nulls and once with"""
    rng = np.random.default_rng([seed, n])
    cols, names = [], []
    for p_null, tag in ((0.0, "full"), (0.2, "nulls")):
        for t in TYPES:
            cols.append(random_column(rng, t, n, p_null))
            names.append(f"{t}_{tag}")
        for t in TEMPORAL:
            cols.append(temporal_column(rng, t, n, p_null))
            names.append(f"{t}_{tag}")
        words = pa.array(["w%d" % i for i in range(37)] + [None])
        stamps = pa.array(np.arange(100, 120), pa.int64()).view(pa.timestamp("ms", tz="UTC"))
        for it in (pa.int8(), pa.uint16(), pa.int32(), pa.int64()):
            cols.append(dictionary_column(rng, it, words, n, p_null))
            names.append(f"dict_{it}_{tag}")
        cols.append(dictionary_column(rng, pa.uint8(), stamps, n, p_null))
        names.append(f"dict_stamps_{tag}")
    return pa.table(cols, names=names)


def device_columns(sess, table):
    return [ac.DeviceArray(sess, sess._import(c.combine_chunks() if isinstance(c, pa.ChunkedArray) else c)) for c in table.columns]


@pytest.fixture(scope="module")
def streams(sess):
    """(rows, compression) → (table, stream, write stats), written once"""
    cache = {}

    def get(rows, compression):
        if (rows, compression) not in cache:
            if rows not in cache:
                t = all_types_table(rows)
                cache[rows] = (t, device_columns(sess, t))
            t, cols = cache[rows]
            buf = sess.write_ipc(t.column_names, [cols], compression=compression)
            cache[(rows, compression)] = (t, buf, dict(sess.last_ipc_write_stats))
        return cache[(rows, compression)]

    return get


@pytest.mark.parametrize("compression", ["lz4", "none"])
@pytest.mark.parametrize("rows", ROWS)
def test_round_trip_through_pyarrow(streams, rows, compression):
    table, buf, stats = streams(rows, compression)
    got = pa.ipc.open_stream(buf).read_all()
    assert got.schema.equals(table.schema), got.schema       # types, time zones, dictionary index types
    assert got.num_rows == rows
    for name in table.column_names:
        a, e = got.column(name), table.column(name)
        assert a.type == e.type and a.null_count == e.null_count and a.equals(e), name


@pytest.mark.parametrize("compression", ["lz4", "none"])
@pytest.mark.parametrize("rows", ROWS)
def test_round_trip_through_this_reader(sess, streams, rows, compression):
    table, buf, stats = streams(rows, compression)
    got = list(sess.read_ipc(buf))
    read_stats = dict(sess.last_ipc_stats)
    assert len(got) == 1
    names, cols, n = got[0]
    assert names == table.column_names and n == rows
    for name, c in zip(names, cols):
        a, e = c.to_arrow(), table.column(name).combine_chunks()
        assert a.type == e.type and a.equals(e), name
    if compression == "lz4":
        assert read_stats["device_fallbacks"] == 0 and read_stats["host_buffers"] == 0      # no frame the device decoder refuses
        if rows >= 1000:
            assert read_stats["device_buffers"] > 0 and stats["buffers_compressed"] > 0
            assert read_stats["device_buffers"] == stats["buffers_compressed"]


# ---- walking a stream: the framing, the metadata's buffer table, every buffer back to its plain bytes ---------------------------------
def walk(stream):
    """[(header type, rows, [(offset, length)], body bytes, compressed)] per message, the end-of-stream marker checked"""
    out, at = [], 0
    while True:
        word, mlen = struct.unpack_from("<Ii", stream, at)
        assert word == 0xFFFFFFFF and at % 8 == 0
        if mlen == 0:
            assert at + 8 == len(stream)
            return out
        assert mlen % 8 == 0
        meta = stream[at + 8:at + 8 + mlen]
        msg = struct.unpack_from("<I", meta, 0)[0]
        kind = meta[R._field(meta, msg, 1)]
        blen_at = R._field(meta, msg, 3)
        blen = struct.unpack_from("<q", meta, blen_at)[0] if blen_at else 0
        body = stream[at + 8 + mlen:at + 8 + mlen + blen]
        assert len(body) == blen and blen % 8 == 0
        at += 8 + mlen + blen
        rb = R._indirect(meta, msg, 2) if kind == R.HEADER_RECORD_BATCH else R._indirect(meta, R._indirect(meta, msg, 2), 1) if kind == R.HEADER_DICTIONARY_BATCH else 0
        bufs, rows, compressed = [], 0, False
        if rb:
            rows = struct.unpack_from("<q", meta, R._field(meta, rb, 0))[0]
            bv = R._indirect(meta, rb, 2)
            bufs = [struct.unpack_from("<qq", meta, bv + 4 + 16 * i) for i in range(struct.unpack_from("<I", meta, bv)[0])]
            compressed = R._field(meta, rb, 3) != 0
        out.append((kind, rows, bufs, body, compressed))


def plain_buffers(message):
    """the buffers of one message inflated, with the layout rules checked: ascending 8-aligned offsets, zero padding, a frame of the
    kind the device reader takes or raw bytes behind -1 → [(plain bytes, how)] with how in 'empty', 'frame', 'raw', 'plain'"""
    kind, rows, bufs, body, compressed = message
    out, end = [], 0
    for off, ln in bufs:
        if ln == 0:
            out.append((b"", "empty"))
            continue
        assert off % 8 == 0 and off >= end and body[end:off] == bytes(off - end), "padding is zero"
        end = off + ln
        piece = body[off:end]
        if not compressed:
            out.append((piece, "plain"))
            continue
        ulen = struct.unpack_from("<q", piece, 0)[0]
        if ulen == -1:
            out.append((piece[8:], "raw"))
            continue
        flg, bd, blocks, stop = M.parse_frame(piece[8:])
        assert piece[8:12] == struct.pack("<I", M.MAGIC) and flg == 0x60 and bd == 0x40 and piece[14] == (M.xxh32(piece[12:14]) >> 8) & 0xFF
        assert 8 + stop == ln and len(piece) - 8 < ulen, "a frame is written only where it is smaller"
        plain = b""
        for i, (data, stored) in enumerate(blocks):
            want = min(65536, ulen - 65536 * i)
            plain += data if stored else M.decode_block(data, want)
            assert len(plain) == min(ulen, 65536 * (i + 1))
        assert len(plain) == ulen
        out.append((plain, "frame"))
    assert body[end:] == bytes(len(body) - end)
    return out


def check_trailing_bits(stream):
    """every bit past `rows` in a written bitmap (validity, boolean data) is zero; → number of bitmaps looked at"""
    schema = pa.ipc.open_stream(stream).schema
    dict_fields = [f for f in schema if pa.types.is_dictionary(f.type)]
    seen = 0
    for message in walk(stream):
        kind, rows, bufs, body, compressed = message
        if kind == R.HEADER_RECORD_BATCH:
            types = [f.type.index_type if pa.types.is_dictionary(f.type) else f.type for f in schema]
        elif kind == R.HEADER_DICTIONARY_BATCH:
            types = None     # one column of a value type: only its validity is a bitmap
        else:
            continue
        plains = plain_buffers(message)
        if types is None:
            columns = [(len(plains), [0])]
        else:
            var = lambda t: pa.types.is_string(t) or pa.types.is_binary(t) or pa.types.is_large_string(t) or pa.types.is_large_binary(t)
            columns = [(3 if var(t) else 2, [0, 1] if pa.types.is_boolean(t) else [0]) for t in types]
        at = 0
        for nbuf, bitmaps in columns:
            for k in bitmaps:
                bm = plains[at + k][0]
                if not bm:
                    continue
                assert len(bm) == (rows + 7) // 8
                assert not np.unpackbits(np.frombuffer(bm, np.uint8), bitorder="little")[rows:].any()
                seen += 1
            at += nbuf
        assert at == len(plains)
    return seen


@pytest.mark.parametrize("compression", ["lz4", "none"])
@pytest.mark.parametrize("cut", [3, 67])
def test_slices_are_written_as_their_offset_zero_copies(sess, compression, cut):
    rng = np.random.default_rng(cut)
    n = 100
    base = [random_column(rng, pa.int64(), 300, 0.2), random_column(rng, pa.bool_(), 300, 0.2), random_column(rng, pa.string(), 300, 0.2),
            random_column(rng, pa.bool_(), 300, 0.0), dictionary_column(rng, pa.int32(), pa.array(["a", "bb", "ccc"]), 300, 0.1)]
    names = ["i", "b", "s", "bf", "d"]
    sliced = [c.slice(cut, n) for c in base]
    assert all(c.offset == cut for c in sliced)
    copies = [pa.concat_arrays([c]) if not pa.types.is_dictionary(c.type) else pa.DictionaryArray.from_arrays(pa.concat_arrays([c.indices]), c.dictionary)
              for c in sliced]
    assert all(c.offset == 0 for c in copies)
    a = sess.write_ipc(names, [[ac.DeviceArray(sess, sess._import(c)) for c in sliced]], compression=compression)
    b = sess.write_ipc(names, [[ac.DeviceArray(sess, sess._import(c)) for c in copies]], compression=compression)
    assert a == b
    got = pa.ipc.open_stream(a).read_all()
    for name, e in zip(names, sliced):
        assert got.column(name).combine_chunks().equals(e), name
    assert check_trailing_bits(a) >= 4


@pytest.mark.parametrize("compression", ["lz4", "none"])
def test_every_byte_of_the_stream_is_defined(sess, compression):
    table = all_types_table(1003, seed=4)
    cols = device_columns(sess, table)
    first = sess.write_ipc(table.column_names, [cols, cols], compression=compression)
    # dirty what the writer's temporaries are made of: blocks of the pool filled with ones and given back, and another call's scratch
    junk = [ac.DeviceArray(sess, sess._import(pa.array(np.full(1 << 18, -1, np.int64)))) for _ in range(4)]
    sess.call_function("unique", [junk[0]])
    sess.call_function("unique", [cols[table.column_names.index("string_nulls")]])
    for j in junk:
        j.release()
    second = sess.write_ipc(table.column_names, [cols, cols], compression=compression)
    assert first == second
    messages = walk(first)
    assert [m[0] for m in messages].count(R.HEADER_RECORD_BATCH) == 2
    for m in messages:
        plain_buffers(m)
    assert check_trailing_bits(first) > 40


def test_incompressible_and_empty_buffers(sess):
    rng = np.random.default_rng(12)
    n = 20000
    noise = pa.array(rng.random(n))                          # 52 random mantissa bits per value: no frame is smaller
    steps = pa.array(np.arange(n, dtype=np.int64))
    t = pa.table([noise, steps, random_column(rng, pa.string(), n, 0.0)], names=["noise", "steps", "s"])
    buf = sess.write_ipc(t.column_names, [device_columns(sess, t)], compression="lz4")
    stats = dict(sess.last_ipc_write_stats)
    messages = walk(buf)
    hows = [how for _, how in plain_buffers(messages[1])]      # noise: validity, data; steps: validity, data; s: validity, offsets, data
    assert hows[:4] == ["empty", "raw", "empty", "frame"] and hows[4] == "empty" and hows[6] == "frame"   # null count 0: no validity bytes
    assert stats["buffers_raw"] == hows.count("raw") and stats["buffers_compressed"] == hows.count("frame")
    assert stats["raw_bytes"] > stats["body_bytes"] > 8 * n
    assert pa.ipc.open_stream(buf).read_all().equals(t)
    names, cols, rows = next(iter(sess.read_ipc(buf)))
    assert all(c.to_arrow().equals(t.column(k).combine_chunks()) for k, c in zip(names, cols))
    # a batch of no rows: every buffer has length 0, with and without compression
    empty = t.slice(0, 0)
    for compression in ("lz4", "none"):
        buf = sess.write_ipc(t.column_names, [device_columns(sess, empty)], compression=compression)
        messages = walk(buf)
        assert messages[1][1] == 0 and all(ln == 0 for _, ln in messages[1][2]) and len(messages[1][3]) == 0
        assert pa.ipc.open_stream(buf).read_all().equals(empty)


def test_dictionaries_are_written_once_and_replaced(sess):
    rng = np.random.default_rng(2)
    words, other = pa.array(["w%d" % i for i in range(30)]), pa.array(["other%d" % i for i in range(9)] + [None])
    k = dictionary_column(rng, pa.int16(), words, 500, 0.1)
    schema = pa.schema([("k", k.type), ("x", pa.int32())])
    b1 = pa.record_batch([k, pa.array(np.arange(500, dtype=np.int32))], schema=schema)
    b2 = b1.slice(100, 70)
    b3 = pa.record_batch([dictionary_column(rng, pa.int16(), other, 40, 0.0), pa.array(np.arange(40, dtype=np.int32))], schema=schema)
    sink = pa.BufferOutputStream()
    with pa.ipc.new_stream(sink, schema) as w:
        w.write_batch(b1)
        w.write_batch(b2)
    shared = [cols for _, cols, _ in sess.read_ipc(sink.getvalue())]             # two batches over ONE dictionary in HBM
    third = [ac.DeviceArray(sess, sess._import(c)) for c in b3.columns]
    for compression in ("lz4", "none"):
        buf = sess.write_ipc(["k", "x"], shared + [third], compression=compression)
        kinds = [m[0] for m in walk(buf)]
        assert kinds == [1, R.HEADER_DICTIONARY_BATCH, R.HEADER_RECORD_BATCH, R.HEADER_RECORD_BATCH, R.HEADER_DICTIONARY_BATCH, R.HEADER_RECORD_BATCH]
        got = list(pa.ipc.open_stream(buf))
        assert len(got) == 3
        for g, e in zip(got, (b1, b2, b3)):
            assert g.schema.equals(schema) and g.equals(e)
        back = [[c.to_arrow() for c in cols] for _, cols, _ in sess.read_ipc(buf)]
        assert all(a.equals(e) for cols, b in zip(back, (b1, b2, b3)) for a, e in zip(cols, b.columns))


def test_errors_leave_the_writer_and_the_session_usable(sess):
    import ctypes as C
    import decimal
    lib = ac.lib
    good = pa.table([pa.array([1, 2, 3], pa.int64()), pa.array(["a", None, "c"])], names=["i", "s"])
    cols = device_columns(sess, good)

    def write(w, names, arrays):
        cn = (C.c_char_p * len(names))(*[n.encode() for n in names])
        hs = (C.c_void_p * len(arrays))(*[a.h for a in arrays])
        sess._check(lib.ahc_ipc_write_batch(w, len(names), cn, hs))

    w = C.c_void_p()
    with pytest.raises(ac.ErrInvalid, match="compression"):
        sess._check(lib.ahc_ipc_writer_open(sess.h, b"compression=zstd", C.byref(w)))
    sess._check(lib.ahc_ipc_writer_open(sess.h, b"compression=lz4", C.byref(w)))
    try:
        with pytest.raises(ac.ErrNotImplemented, match="'price'"):          # an unsupported type, before any schema exists
            write(w, ["i", "price"], [cols[0], ac.DeviceArray(sess, sess._import(pa.array([decimal.Decimal("1.25")] * 3, pa.decimal128(9, 2))))])
        write(w, ["i", "s"], cols)
        with pytest.raises(ac.ErrInvalid, match="'s'"):                      # another type for a column of the schema
            write(w, ["i", "s"], [cols[0], cols[0]])
        with pytest.raises(ac.ErrInvalid, match="'t'"):                      # another name
            write(w, ["i", "t"], cols)
        with pytest.raises(ac.ErrInvalid, match="'s'.*chunk by chunk"):
            write(w, ["i", "s"], [cols[0], ac.DeviceArray(sess, sess._import(pa.chunked_array([["a"], ["b", "c"]])))])
        with pytest.raises(ac.ErrInvalid, match="'s' has 2 rows"):
            write(w, ["i", "s"], [cols[0], ac.DeviceArray(sess, sess._import(pa.array(["a", "b"])))])
        write(w, ["i", "s"], cols)
        p, n = C.c_void_p(), C.c_int64()
        sess._check(lib.ahc_ipc_writer_finish(w, C.byref(p), C.byref(n)))
        buf = C.string_at(p.value, n.value)
    finally:
        lib.ahc_ipc_writer_close(w)
    got = list(pa.ipc.open_stream(buf))
    assert len(got) == 2 and all(pa.Table.from_batches([g]).equals(good) for g in got)
    with pytest.raises(ac.ErrInvalid, match="chunk by chunk"):               # a scalar datum
        sess.write_ipc(["i"], [[ac.DeviceArray(sess, sess._scalar(pa.scalar(1, pa.int64())))]])
    with pytest.raises(ValueError):
        sess.write_ipc(["i"], [[cols[0]]], compression="zstd")
    assert sess.call_function("add_unchecked", [cols[0], cols[0]]).to_pylist() == [2, 4, 6]
