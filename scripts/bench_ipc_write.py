"""Session.write_ipc: record batches leave HBM as an IPC stream, compressed on the device.

Two parts, written to two keys of profiles/ipc_write_lz4.json (the other key of an existing file is kept):

  --ratios   no GPU: the block compressor's sizes against liblz4's (pyarrow's "lz4_raw" codec) on the corpora of
             tests/lz4_enc_vectors.py, through the host harness (tests/lz4_enc_harness.cc: csrc/ah_lz4_enc.h with its lanes in a loop,
             the same bytes the device writes).  A measurement, not a bar.
  (default)  on the GPU: one 2^LOG2-row batch of four columns — an Int64 counter, Float64 random values, a low-cardinality string
             column, an Int32 column with 10 % nulls — WARMUP untimed and REPS timed runs each of
               compress  ah_lz4_compress_blocks alone over each column's plain bytes already in HBM (stream events around the call:
                         the kernel plus its table upload, size download and synchronisation — an upper bound of the kernel's time)
               pack      ah_ipc_pack_body alone moving the same bytes as plain pieces
               write     Session.write_ipc of the batch, compression "lz4" and "none", wall time
               pyarrow   the path a user has without the writer: every column downloaded (to_arrow), then pyarrow's IPC writer with
                         compression="lz4" on the host; the download and the host writer are timed separately
             medians with min – max, and compressed / raw per column.

    python scripts/bench_ipc_write.py [--ratios] [--log2 24] [--reps 10] [--warmup 2] [--out profiles/ipc_write_lz4.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import pyarrow as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import lz4_enc_vectors as EV  # noqa: E402
from tests import lz4_model as M  # noqa: E402
from tests.test_lz4_enc_host import build_harness, compress_lines, compressed  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ratios", action="store_true")
ap.add_argument("--log2", type=int, default=24)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ipc_write_lz4.json"))
args = ap.parse_args()
BLOCK = 65536


def stat(xs):
    xs = sorted(xs)
    return {"median": round(statistics.median(xs), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def save(key, value):
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc[key] = value
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("written:", args.out, "/", key)


def ratios():
    with tempfile.TemporaryDirectory(prefix="lz4_enc_harness_") as d:
        run = build_harness(d)
        vecs = [(name, data) for name, data in EV.vectors() if len(data) >= 4095]
        answers = [compressed(a) for a in run(compress_lines([data for _, data in vecs]))]
    rows, ours_total, lib_total, raw_total = {}, 0, 0, 0
    for (name, data), (stored, _size, out) in zip(vecs, answers):
        ref = len(pa.Codec("lz4_raw").compress(data))
        ref = min(ref, len(data))          # a block that does not shrink is stored by either
        assert out == data if stored else M.decode_block(out, len(data)) == data
        rows[name] = {"raw": len(data), "this": len(out), "liblz4": ref, "this_over_liblz4": round(len(out) / ref, 3)}
        ours_total += len(out)
        lib_total += ref
        raw_total += len(data)
    save("block_sizes_against_liblz4", {
        "what": "scripts/bench_ipc_write.py --ratios: bytes of one LZ4 block per corpus of tests/lz4_enc_vectors.py (>= 4095 bytes), "
                "csrc/ah_lz4_enc.h through the host harness against liblz4 (pyarrow lz4_raw); a stored block counts its raw size",
        "total": {"raw": raw_total, "this": ours_total, "liblz4": lib_total, "this_over_liblz4": round(ours_total / lib_total, 3)},
        "corpora": rows})


def bench():
    import arrow_go_amd as ah
    from arrow_go_amd import compute as ac
    if ah.device_count() < 1:
        raise SystemExit("bench_ipc_write: no GPU visible")
    n = 1 << args.log2
    rng = np.random.default_rng(1)
    words = np.array(["alpha", "beta", "gamma-ray", "delta", "epsilon", "zeta", "eta", "theta"])
    table = pa.table({
        "counter": pa.array(np.arange(n, dtype=np.int64)),
        "noise": pa.array(rng.random(n)),
        "word": pa.array(words[rng.integers(0, len(words), n)]),
        "sparse": pa.array(rng.integers(0, 1000, n, dtype=np.int32), mask=rng.random(n) < 0.1),
    })
    sess = ac.Session(0)
    ctx = ah.Context(0)
    cols = [ac.DeviceArray(sess, sess._import(c.combine_chunks())) for c in table.columns]
    res = {"what": "scripts/bench_ipc_write.py: one batch of 2^%d rows {Int64 counter, Float64 random, low-cardinality string, Int32 with 10 %% "
                   "nulls}; ms as median (min, max) of %d runs after %d warm-ups" % (args.log2, args.reps, args.warmup),
           "rows": n, "reps": args.reps, "warmup": args.warmup, "columns": {}}

    # ---- the two kernels alone, per column, over the plain bytes of the column's largest buffer ------------------------------------
    for name in table.column_names:
        arr = table.column(name).combine_chunks()
        plain = np.frombuffer(arr.buffers()[-1], np.uint8)
        nblocks = -(-len(plain) // BLOCK)
        blocks = np.array([(i * BLOCK, min(BLOCK, len(plain) - i * BLOCK), i * BLOCK) for i in range(nblocks)], np.int64)
        dsrc, dcomp, dout = ctx.to_device(plain, pad=16), ctx.alloc(len(plain) + 16), ctx.alloc(len(plain) + 16)
        ks, ps = [], []
        rows = np.array([(i * BLOCK, min(BLOCK, len(plain) - i * BLOCK), i * BLOCK, 1) for i in range(nblocks)], np.int64)
        for i in range(args.warmup + args.reps):
            ctx.timer_start()
            sizes, stored = ctx.lz4_compress_blocks(dsrc, len(plain), dcomp, len(plain), blocks)
            ms = ctx.timer_stop()
            ctx.timer_start()
            ctx.ipc_pack_body(dcomp, len(plain), dsrc, len(plain), b"", rows, dout, len(plain))
            pms = ctx.timer_stop()
            if i >= args.warmup:
                ks.append(ms)
                ps.append(pms)
        assert dout.download(np.uint8, min(len(plain), 1 << 20)).tobytes() == plain[:1 << 20].tobytes()
        for b in (dsrc, dcomp, dout):
            b.free()
        res["columns"][name] = {
            "plain_bytes": int(len(plain)), "blocks": int(nblocks), "blocks_stored": int(stored.sum()),
            "compressed_over_raw": round(float(sizes.sum()) / len(plain), 4),
            "compress_call_ms": stat(ks), "compress_gb_per_s_plain": round(len(plain) / 1e6 / statistics.median(ks), 2),
            "pack_call_ms": stat(ps), "pack_gb_per_s": round(len(plain) / 1e6 / statistics.median(ps), 2)}
        print(name, json.dumps(res["columns"][name]), flush=True)

    # ---- the whole write, and the path a user has today ---------------------------------------------------------------------------------
    def timed(f):
        t0 = time.perf_counter()
        out = f()
        return (time.perf_counter() - t0) * 1e3, out

    t = {"lz4": [], "none": [], "download": [], "pyarrow_lz4": []}
    sizes = {}
    for i in range(args.warmup + args.reps):
        for compression in ("lz4", "none"):
            ms, buf = timed(lambda: sess.write_ipc(table.column_names, [cols], compression=compression))
            sizes[compression] = len(buf)
            if compression == "lz4":
                res["write_stats_lz4"] = dict(sess.last_ipc_write_stats)
            if i == 0:
                assert pa.ipc.open_stream(buf).read_all().equals(table), compression
            del buf
            if i >= args.warmup:
                t[compression].append(ms)
        dms, host = timed(lambda: [c.to_arrow() for c in cols])

        def host_write():
            sink = pa.BufferOutputStream()
            with pa.ipc.new_stream(sink, table.schema, options=pa.ipc.IpcWriteOptions(compression="lz4")) as w:
                w.write_batch(pa.record_batch(host, names=table.column_names))
            return sink.getvalue().size

        pms, size = timed(host_write)
        sizes["pyarrow_lz4"] = size
        if i >= args.warmup:
            t["download"].append(dms)
            t["pyarrow_lz4"].append(pms)
    res["write_ipc_lz4_ms"] = stat(t["lz4"])
    res["write_ipc_none_ms"] = stat(t["none"])
    res["download_columns_ms"] = stat(t["download"])
    res["pyarrow_host_writer_lz4_ms"] = stat(t["pyarrow_lz4"])
    res["download_plus_pyarrow_lz4_ms"] = round(res["download_columns_ms"]["median"] + res["pyarrow_host_writer_lz4_ms"]["median"], 4)
    res["stream_bytes"] = sizes
    res["lz4_over_none"] = round(res["write_ipc_lz4_ms"]["median"] / res["write_ipc_none_ms"]["median"], 3)
    print(json.dumps({k: v for k, v in res.items() if k != "columns"}), flush=True)
    save("write_batch", res)


if args.ratios:
    ratios()
else:
    bench()
