"""LZ4-frame record-batch bodies inflated in HBM: ah_lz4_decompress_blocks on the block vectors the host harness of
tests/test_lz4_host.py has already decoded under sanitizers (run that file first), and Session.read_ipc on streams whose buffers are
frames of independent blocks (tests/ipc_rewrite.py makes them from pyarrow's) against the host path of the same build
(ipc_device_lz4 = 0) and against pyarrow."""
import struct

import numpy as np
import pyarrow as pa
import pytest

from arrow_go_amd import compute as ac
from tests import ipc_rewrite as R
from tests import lz4_model as M
from tests import lz4_vectors as V
from tests.test_ipc import TYPES, random_column

pytestmark = pytest.mark.gpu
GUARD = 64
STORED = 1 << 62


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def run_blocks(ctx, blocks, dst_align=0):
    """blocks: [(block bytes, stored, dst_len)] laid out back to back with GUARD bytes of 0xA5 around every output range (and odd
    source positions).  → (status array, [output bytes per block], guards intact)"""
    src, table, dst_at = bytearray(b"\x5a" * 3), [], GUARD + dst_align
    for data, stored, dst_len in blocks:
        table.append((len(src), len(data) | (STORED if stored else 0), dst_at, dst_len))
        src += data + b"\x5a" * (len(data) % 3)
        dst_at += dst_len + GUARD
    dsrc = ctx.to_device(np.frombuffer(bytes(src), np.uint8), pad=16)
    ddst = ctx.alloc(dst_at + 16)
    ddst.memset(0xA5)
    status = ctx.lz4_decompress_blocks(dsrc, len(src), ddst, dst_at, table)
    host = ddst.download(np.uint8, dst_at).tobytes()
    outs, guards_ok, prev_end = [], True, 0
    for (_, _, d0, dl) in table:
        guards_ok &= host[prev_end:d0] == b"\xa5" * (d0 - prev_end)
        outs.append(host[d0:d0 + dl])
        prev_end = d0 + dl
    guards_ok &= host[prev_end:] == b"\xa5" * (dst_at - prev_end)
    dsrc.free()
    ddst.free()
    return status, outs, guards_ok


@pytest.mark.parametrize("dst_align", [0, 5])
def test_sequence_vectors(ctx, dst_align):
    vecs = V.sequence_vectors()
    status, outs, guards_ok = run_blocks(ctx, [(src, stored, n) for _, src, stored, n in vecs], dst_align)
    assert guards_ok
    for vec, st, out in zip(vecs, status, outs):
        want = V.expected(vec)
        if want is None:
            assert st != 0, vec[0]
        else:
            assert st == 0 and out == want, (vec[0], int(st))


def test_mutated_and_damaged_blocks_end_as_statuses(ctx):
    """the vectors the harness decoded without a sanitizer report: on the device each is a status or the model's bytes, and no byte
    outside a block's own output range changes"""
    vecs = V.mutation_vectors(2000) + [(k, s, False, n) for k, (s, n) in V.damaged_blocks().items()]
    status, outs, guards_ok = run_blocks(ctx, [(src, stored, n) for _, src, stored, n in vecs])
    assert guards_ok
    for vec, st, out in zip(vecs, status, outs):
        want = V.expected(vec)
        assert (st == 0 and out == want) if want is not None else st != 0, vec[0]
    assert all(status[-5:] != 0)


@pytest.fixture(scope="module")
def contents():
    rng = np.random.default_rng(11)
    n = 3 * 65536 + 5
    return {"compressible": rng.integers(0, 4, n, dtype=np.uint8).tobytes(), "stored": rng.integers(0, 256, n, dtype=np.uint8).tobytes(),
            "mixed": b"".join(rng.integers(0, 256 if k % 2 else 3, 30000, dtype=np.uint8).tobytes() for k in range(7))[:n]}


@pytest.mark.parametrize("kind", ["compressible", "stored", "mixed"])
def test_multi_block_pieces(ctx, contents, kind):
    """pieces of 0, 1, 65535, 65536, 65537 and 3·65536 + 5 bytes cut into 64 KiB blocks, all in one call"""
    blocks, want = [], []
    for n in (0, 1, 65535, 65536, 65537, 3 * 65536 + 5):
        data = contents[kind][:n]
        for (b, stored), at in zip(M.split_blocks(data, compress=R.raw_block), range(0, n, 65536)):
            blocks.append((b, stored, min(65536, n - at)))
            want.append(data[at:at + 65536])
    # (pieces of a few bytes travel stored whatever the content: a block of one literal is two bytes)
    assert any(s for _, s, _ in blocks) and any(not s for _, s, _ in blocks) == (kind != "stored")
    status, outs, guards_ok = run_blocks(ctx, blocks)
    assert guards_ok and not status.any() and outs == want
    # a wrong length is a status, and only that block's
    b, stored, n = blocks[3]
    status, outs, guards_ok = run_blocks(ctx, blocks[:3] + [(b, stored, n - 1)] + blocks[4:6])
    assert guards_ok and list(status != 0) == [False, False, False, True, False, False] and outs[4] == want[4]


def test_table_is_validated_before_the_launch(ctx):
    import arrow_go_amd as ah
    src, dst = ctx.to_device(np.zeros(256, np.uint8)), ctx.alloc(1 << 17)
    for table in ([(0, 257, 0, 10)], [(250, 10, 0, 10)], [(0, 10, 0, 65537)], [(0, 10, (1 << 17) - 5, 10)], [(0, 10, 100, 10), (0, 10, 105, 10)],
                  [(-1, 10, 0, 10)], [(0, 10, -1, 10)], [(0, 10, 0, -1)]):
        with pytest.raises(ah.ErrInvalid):
            ctx.lz4_decompress_blocks(src, 256, dst, 1 << 17, table)
    assert len(ctx.lz4_decompress_blocks(src, 256, dst, 1 << 17, [])) == 0
    src.free()
    dst.free()


# ---- the reader -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sess():
    s = ac.Session(0)
    s.set_option("ipc_device_lz4_min_bytes", 0)    # the streams here are small: what is under test is the path, not its threshold
    yield s
    s.set_option("ipc_device_lz4", 1)
    s.close()


def lz4_stream(batches, schema):
    sink = pa.BufferOutputStream()
    with pa.ipc.new_stream(sink, schema, options=pa.ipc.IpcWriteOptions(compression="lz4")) as w:
        for b in batches:
            w.write_batch(b)
    return sink.getvalue().to_pybytes()


def read_all(sess, stream, device):
    """→ ([[bytes of every exported buffer] per column] per batch, [pyarrow arrays per batch], stats)"""
    sess.set_option("ipc_device_lz4", int(device))
    raw, arrays = [], []
    for names, cols, rows in sess.read_ipc(stream):
        arrs = [c.to_arrow() for c in cols]
        arrays.append(arrs)
        raw.append([[None if b is None else b.to_pybytes() for b in a.buffers()] for a in arrs])
    return raw, arrays, dict(sess.last_ipc_stats)


@pytest.fixture(scope="module")
def typed_stream():
    rng = np.random.default_rng(21)
    schema = pa.schema([pa.field("c%d_%s" % (i, t), t) for i, t in enumerate(TYPES)])
    batches = [pa.record_batch([random_column(rng, t, n, 0.2) for t in TYPES], schema=schema) for n in (0, 7, 40000)]
    return schema, batches, R.rewrite(lz4_stream(batches, schema))


def test_device_and_host_paths_agree_on_all_types(sess, typed_stream):
    schema, batches, stream = typed_stream
    assert len(TYPES) == 15
    assert [pa.ipc.open_stream(stream).read_all().equals(pa.Table.from_batches(batches, schema))] == [True]   # the helper's streams are streams
    host_raw, host_arrays, host_stats = read_all(sess, stream, device=False)
    dev_raw, dev_arrays, dev_stats = read_all(sess, stream, device=True)
    assert dev_raw == host_raw
    assert [len(a) for a in dev_arrays] == [len(TYPES)] * 3
    for arrs, b in zip(dev_arrays, batches):
        for got, exp in zip(arrs, b.columns):
            assert got.equals(exp)
    assert host_stats["device_buffers"] == 0 and host_stats["device_fallbacks"] == 0 and host_stats["host_buffers"] > 0
    assert dev_stats["device_buffers"] > 0 and dev_stats["device_fallbacks"] == 0
    assert dev_stats["device_buffers"] + dev_stats["host_buffers"] == host_stats["host_buffers"]
    assert dev_stats["bytes_uploaded"] < host_stats["bytes_uploaded"]       # the compressed bytes crossed the link


def one_column_stream(n=100000, seed=5):
    """an Int64 column without nulls: one data buffer of n·8 bytes (13 blocks), no validity buffer"""
    rng = np.random.default_rng(seed)
    col = pa.array(rng.integers(0, 50, n), pa.int64())
    schema = pa.schema([pa.field("v", pa.int64(), nullable=False)])
    return col, lz4_stream([pa.record_batch([col], schema=schema)], schema)


def first_frame_flg(stream, n_bytes):
    at = stream.index(struct.pack("<q", n_bytes) + struct.pack("<I", M.MAGIC))
    return stream[at + 12]


def test_an_untouched_pyarrow_stream_stays_on_the_host(sess):
    col, stream = one_column_stream()
    assert not first_frame_flg(stream, 800000) & M.FLG_INDEP       # Arrow C++ links the blocks of a frame beyond one block
    raw, arrays, stats = read_all(sess, stream, device=True)
    assert arrays[0][0].equals(col) and stats["device_buffers"] == 0 and stats["device_fallbacks"] == 0 and stats["host_buffers"] == 1


def test_threshold_keeps_small_bodies_on_the_host(sess):
    col, stream = one_column_stream()
    stream = R.rewrite(stream)
    assert first_frame_flg(stream, 800000) & M.FLG_INDEP
    try:
        sess.set_option("ipc_device_lz4_min_bytes", 1 << 30)
        assert read_all(sess, stream, device=True)[2]["device_buffers"] == 0
    finally:
        sess.set_option("ipc_device_lz4_min_bytes", 0)
    raw, arrays, stats = read_all(sess, stream, device=True)
    assert arrays[0][0].equals(col) and stats["device_buffers"] == 1 and stats["host_buffers"] == 0


def test_a_short_middle_block_falls_back_once(sess):
    col, stream = one_column_stream()
    assert -(-800000 // 65536) == 13

    def short_middle(plain, index, stored):
        sizes = [65536, 60000] + [65536] * 10
        sizes.append(len(plain) - sum(sizes))
        assert 0 < sizes[-1] <= 65536 and len(sizes) == 13
        blocks, at = [], 0
        for s in sizes:
            blocks += M.split_blocks(plain[at:at + s], compress=R.raw_block)
            at += s
        return M.frame(blocks)

    stream = R.rewrite(stream, short_middle)
    assert pa.ipc.open_stream(stream).read_all().column(0).chunk(0).equals(col)
    raw, arrays, stats = read_all(sess, stream, device=True)
    assert arrays[0][0].equals(col)
    assert stats["device_fallbacks"] == 1 and stats["device_buffers"] == 0 and stats["host_buffers"] == 0


def test_a_frame_with_a_content_checksum_goes_to_the_host(sess):
    col, stream = one_column_stream()
    stream = R.rewrite(stream, lambda plain, index, stored: M.frame(M.split_blocks(plain, compress=R.raw_block),
                                                                    flg=M.FLG_VERSION | M.FLG_INDEP | M.FLG_CONTENT_CHECKSUM, content=plain))
    raw, arrays, stats = read_all(sess, stream, device=True)
    assert arrays[0][0].equals(col) and stats == dict(stats, device_buffers=0, host_buffers=1, device_fallbacks=0)


@pytest.mark.parametrize("name", list(V.damaged_blocks()))
def test_damaged_frames_raise_and_the_session_lives_on(sess, name):
    """a frame that qualifies by its header around a block that is wrong in one way: ErrInvalid, and the next read works"""
    block, n = V.damaged_blocks()[name]
    col = pa.array(np.arange(n) % 7, pa.uint8())
    schema = pa.schema([pa.field("v", pa.uint8(), nullable=False)])
    stream = R.rewrite(lz4_stream([pa.record_batch([col], schema=schema)], schema), lambda plain, index, stored: M.frame([(block, False)]))
    sess.set_option("ipc_device_lz4", 1)
    with pytest.raises(ac.ErrInvalid):
        list(sess.read_ipc(stream))
    good_col, good = one_column_stream(20000, seed=6)
    raw, arrays, stats = read_all(sess, R.rewrite(good), device=True)
    assert arrays[0][0].equals(good_col) and stats["device_buffers"] == 1
