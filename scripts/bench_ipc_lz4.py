"""Session.read_ipc of LZ4_FRAME bodies: the device inflate (session option ipc_device_lz4 = 1) against the host inflate of the same
build (= 0, the path before the device decoder existed), alternating in one process.

Every stream holds one record batch with one UInt8 column without nulls, whose data buffer is a frame of independent 64 KiB blocks of
2^16 … 2^28 plain bytes.  A frame of independent blocks is a concatenation of block records, so one 64 KiB block is compressed once
(liblz4's block compressor through pyarrow's "lz4_raw" codec) and repeated with numpy.  Two contents: words drawn from a small
vocabulary (compressible) and random bytes whose last 4 KiB repeat the first (near-incompressible, but still a compressed block).
Per size and content: WARMUP untimed reads of each path, then REPS timed pairs; wall time around the whole read (both paths end in a
synchronisation).  "call" is ah_lz4_decompress_blocks alone between two events on the compute stream, the compressed bytes already
in HBM: the kernel plus the call's table upload, status download and synchronisation — an upper bound of the kernel's time.  Writes profiles/ipc_lz4_device.json.

    python scripts/bench_ipc_lz4.py [--max-log2 28] [--reps 10] [--out profiles/ipc_lz4_device.json]
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time

import numpy as np
import pyarrow as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import arrow_go_amd as ah  # noqa: E402
from arrow_go_amd import compute as ac  # noqa: E402
from tests import ipc_rewrite as R  # noqa: E402
from tests import lz4_model as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--min-log2", type=int, default=16)
ap.add_argument("--max-log2", type=int, default=28)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipc_lz4_device.json"))
args = ap.parse_args()
if ah.device_count() < 1:
    raise SystemExit("bench_ipc_lz4: no GPU visible")

BLOCK = 65536
rng = np.random.default_rng(1)
words = [bytes(rng.integers(97, 123, int(rng.integers(3, 12)), dtype=np.uint8)) + b" " for _ in range(400)]
text = b"".join(words[j] for j in rng.integers(0, len(words), 20000))[:BLOCK]
noise = bytearray(rng.integers(0, 256, BLOCK, dtype=np.uint8).tobytes())
noise[-4096:] = noise[:4096]
CONTENTS = {"compressible": text, "near_incompressible": bytes(noise)}


def make_stream(plain_block, nblocks):
    """→ (stream bytes, the column)"""
    comp = R.raw_block(plain_block)
    assert len(comp) < BLOCK and M.decode_block(comp, BLOCK) == plain_block
    col = pa.array(np.tile(np.frombuffer(plain_block, np.uint8), nblocks), pa.uint8())
    schema = pa.schema([pa.field("v", pa.uint8(), nullable=False)])
    sink = pa.BufferOutputStream()
    with pa.ipc.new_stream(sink, schema, options=pa.ipc.IpcWriteOptions(compression="lz4")) as w:
        w.write_batch(pa.record_batch([col], schema=schema))
    record = np.frombuffer(struct.pack("<I", len(comp)) + comp, np.uint8)
    head = M.frame([])[:7]

    def reframe(plain, index, stored):
        assert len(plain) == nblocks * BLOCK
        return head + np.tile(record, nblocks).tobytes() + struct.pack("<I", 0)

    return R.rewrite(sink.getvalue().to_pybytes(), reframe), col, len(comp)


def stat(xs):
    xs = sorted(xs)
    return {"median": round(statistics.median(xs), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


sess = ac.Session(0)
sess.set_option("ipc_device_lz4_min_bytes", 0)
ctx = ah.Context(0)
res = {"what": "scripts/bench_ipc_lz4.py: ms per Session.read_ipc of one LZ4_FRAME buffer of independent 64 KiB blocks; host = ipc_device_lz4 0, "
               "device = 1, alternating; call = ah_lz4_decompress_blocks alone (stream events around the whole call: kernel + table upload + "
               "status download), GB/s of plain bytes",
       "reps": args.reps, "warmup": args.warmup, "results": {}}


def read(stream, device):
    sess.set_option("ipc_device_lz4", device)
    t0 = time.perf_counter()
    got = [cols for _names, cols, _rows in sess.read_ipc(stream)]
    dt = (time.perf_counter() - t0) * 1e3
    return dt, got


for name, block in CONTENTS.items():
    for lg in range(args.min_log2, args.max_log2 + 1):
        nblocks = (1 << lg) // BLOCK
        stream, col, csize = make_stream(block, nblocks)
        for device in (0, 1):     # both paths return the column (checked once per configuration, on the smaller sizes in full)
            _, got = read(stream, device)
            if lg <= 22:
                assert got[0][0].to_arrow().equals(col), (name, lg, device)
            stats = dict(sess.last_ipc_stats)
            assert stats["device_buffers"] == device and stats["host_buffers"] == 1 - device and stats["device_fallbacks"] == 0, stats
            del got
        for _ in range(args.warmup):
            read(stream, 0)
            read(stream, 1)
        t = {0: [], 1: []}
        for _ in range(args.reps):
            for device in (0, 1):
                t[device].append(read(stream, device)[0])
        # the decoder call alone
        table = np.array([(i * (4 + csize) + 4, csize, i * BLOCK, BLOCK) for i in range(nblocks)], np.int64)
        body = np.tile(np.frombuffer(struct.pack("<I", csize) + R.raw_block(block), np.uint8), nblocks)
        dsrc, ddst = ctx.to_device(body), ctx.alloc(nblocks * BLOCK)
        ks = []
        for i in range(args.warmup + args.reps):
            ctx.timer_start()
            status = ctx.lz4_decompress_blocks(dsrc, body.nbytes, ddst, nblocks * BLOCK, table)
            ms = ctx.timer_stop()
            assert not status.any()
            if i >= args.warmup:
                ks.append(ms)
        assert ddst.download(np.uint8, BLOCK, (nblocks - 1) * BLOCK).tobytes() == block
        dsrc.free()
        ddst.free()
        r = {"plain_bytes": nblocks * BLOCK, "compressed_body_bytes": 8 + 7 + nblocks * (4 + csize) + 4, "ratio": round(BLOCK / csize, 3),
             "host_ms": stat(t[0]), "device_ms": stat(t[1]), "call_ms": stat(ks),
             "call_gb_per_s_plain": round(nblocks * BLOCK / 1e6 / statistics.median(ks), 2)}
        r["device_over_host"] = round(r["device_ms"]["median"] / r["host_ms"]["median"], 3)
        res["results"][f"{name}/2^{lg}"] = r
        print(name, lg, json.dumps(r), flush=True)
        del stream, col

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print("written:", args.out)
