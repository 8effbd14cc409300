"""window: what a call costs, beside the two calls that bound it from below on the same data.

One process, one resident record batch per case (g: Int32 partition column, k: Int64 order key, v: Int64 values; every column
uploaded once).  The calls alternate — window with row_number alone, window with all seven functions, sort_indices over the same
keys (the part no design can avoid), group_by sum on the same partitions — `--reps` times after `--warmup` rounds, each call timed
on the host from a drained stream to a drained stream (the results stay on the device; the drain is an export of one result
column through the device interface, which synchronises the stream and copies nothing).  Per case: the median and the spread
(min … max) of each.  There is no speed bar: nothing existed before to compare with.  The JSON goes to --out
(profiles/window_bench.json is the committed run; DESIGN.md §3.7.3 holds its table).

    python scripts/bench_window.py [--out FILE] [--reps 7] [--warmup 2] [--sizes 24,26] [--partitions 0,10,20]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import pyarrow as pa

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arrow_go_amd import compute as ac  # noqa: E402

ALL_SEVEN = ["row_number", "rank", "dense_rank", ("v", "cumulative_sum"), ("v", "cumulative_min"), ("v", "cumulative_max"), ("v", "cumulative_count")]


def resident_batch(sess, columns):
    """a record batch whose columns are uploaded once: a DeviceArray holding a record datum"""
    parts = [sess._import(arr) for arr in columns.values()]
    try:
        d = ac._vp()
        names = (C.c_char_p * len(parts))(*[n.encode() for n in columns])
        handles = (ac._vp * len(parts))(*parts)
        sess._check(ac.lib.ahc_record_from_arrays(sess.h, len(parts), names, handles, C.byref(d)))
        return ac.DeviceArray(sess, d)
    finally:
        for p in parts:
            ac.lib.ahc_datum_release(p)


def drain(sess, result):
    """wait for everything the call enqueued: export the last column of a record (or the array) without a copy"""
    h = result.h
    col = None
    ncols = ac.lib.ahc_record_num_columns(h)
    if ncols > 0:
        c, nm = ac._vp(), C.c_char_p()
        sess._check(ac.lib.ahc_record_column(sess.h, h, ncols - 1, C.byref(nm), C.byref(c)))
        col = ac.DeviceArray(sess, c)
    darr, sch = (col or result).export_device()
    darr.array.release(C.byref(darr.array))
    if sch.release:
        sch.release(C.byref(sch))
    if col is not None:
        col.release()
    result.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "window_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="24,26")
    ap.add_argument("--partitions", default="0,10,20")
    args = ap.parse_args()
    sess = ac.Session(0)
    rng = np.random.default_rng(9)
    results = []
    for lg in [int(x) for x in args.sizes.split(",")]:
        rows = 1 << lg
        k = pa.array(rng.integers(-2**62, 2**62, rows, dtype=np.int64))
        v = pa.array(rng.integers(-2**40, 2**40, rows, dtype=np.int64))
        for lp in [int(x) for x in args.partitions.split(",")]:
            g = pa.array(rng.integers(0, 1 << lp, rows, dtype=np.int64).astype(np.int32) if lp else np.zeros(rows, np.int32))
            batch = resident_batch(sess, {"g": g, "k": k, "v": v})
            for ordered in (True, False):
                order_by = [("k", "asc", "at_end")] if ordered else []
                sort_keys = "sort_keys=0:asc:at_end,1:asc:at_end" if ordered else "sort_keys=0:asc:at_end"
                calls = {
                    "window_row_number": lambda: sess.window(batch, ["g"], order_by, ["row_number"], keep_on_device=True),
                    "window_all_seven": lambda: sess.window(batch, ["g"], order_by, ALL_SEVEN, keep_on_device=True),
                    "sort_indices": lambda: sess.call_function("sort_indices", [batch], sort_keys, keep_on_device=True),
                    "group_by_sum": lambda: sess.group_by(batch, ["g"], [("v", "sum")], keep_on_device=True),
                }
                times = {name: [] for name in calls}
                for rep in range(args.warmup + args.reps):
                    for name, fn in calls.items():
                        t0 = time.perf_counter()   # the stream is drained: every round ends with a drain
                        res = fn()
                        drain(sess, res)
                        ms = (time.perf_counter() - t0) * 1e3
                        if rep >= args.warmup:
                            times[name].append(ms)
                row = {"rows_log2": lg, "partitions_log2": lp, "order_keys": 1 if ordered else 0}
                for name, ts in times.items():
                    row[name] = {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
                results.append(row)
                print(json.dumps(row), flush=True)
            batch.release()
    doc = {"reps": args.reps, "warmup": args.warmup, "unit": "ms per call, host clock, drained stream to drained stream",
           "columns": "g int32 (partition), k int64 random (order key), v int64 (values); results stay on the device", "results": results}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    print(json.dumps({"cases": len(results), "out": args.out}))
    sess.close()


if __name__ == "__main__":
    main()
