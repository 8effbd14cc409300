"""select_k against today's way to the same answer: sort_indices and a (zero-copy) slice of its first k entries.

One process, one resident column per case; the calls alternate — select_k on the automatic route, sort_indices, select_k forced
onto the radix route, select_k forced onto the sort route — `--reps` times after `--warmup` rounds, each call timed on the host
from a drained stream to a drained stream (sort_indices returns with its last passes in flight).  Per (column, k): the median and the spread (min … max) of
each, and `auto_not_slower`: the automatic route's median is within the spread of the repeats of sort_indices.  The JSON goes to
--out (profiles/select_k_bench.json is the committed run; DESIGN.md §3.7.2 holds its table).

    python scripts/bench_select_k.py [--out FILE] [--reps 7] [--warmup 2] [--sizes 27,24]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah  # noqa: E402

N = ah._native


def upload_pieces(buf, draw, rows, piece=1 << 22):
    """`rows` values, every piece of 2^22 drawn on its own: a repeated piece would hand the sort's sampled splitters
    (every 512th row) clusters of equal keys, and sort_indices would leave its normal path"""
    for off in range(0, rows, piece):
        values = draw(min(piece, rows - off))
        buf.upload(values, off * values.itemsize)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "select_k_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="27,24")
    args = ap.parse_args()
    ctx = ah.Context(0)
    rng = np.random.default_rng(9)
    results = []
    for lg in [int(x) for x in args.sizes.split(",")]:
        rows = 1 << lg
        a = ctx.alloc(rows * 8)
        b = ctx.alloc(rows * 4)
        out = ctx.alloc(rows * 8)
        for column in ("int64 random", "float64 normal", "int64 in [0, 1000)", "(int32, int64) two keys"):
            if column == "int64 random":
                upload_pieces(a, lambda m: rng.integers(-2**62, 2**62, m, dtype=np.int64), rows)
                keys = [(N.INT64, a, None, 0, None, 0, False, False)]
            elif column == "float64 normal":
                upload_pieces(a, lambda m: rng.standard_normal(m), rows)
                keys = [(N.FLOAT64, a, None, 0, None, 0, False, False)]
            elif column == "int64 in [0, 1000)":
                upload_pieces(a, lambda m: rng.integers(0, 1000, m, dtype=np.int64), rows)
                keys = [(N.INT64, a, None, 0, None, 0, False, False)]
            else:
                upload_pieces(b, lambda m: rng.integers(0, 10**6, m, dtype=np.int32), rows)
                upload_pieces(a, lambda m: rng.integers(-2**62, 2**62, m, dtype=np.int64), rows)
                keys = [(N.INT32, b, None, 0, None, 0, False, False), (N.INT64, a, None, 0, None, 0, False, False)]
            for k in dict.fromkeys((10, 1 << 10, 1 << 16, 1 << 20, rows // 16, rows // 2)):   # n / 16: where the automatic route changes
                calls = {
                    "select_k_auto": lambda: ctx.select_k(keys, rows, k, out, 0),
                    "sort_indices_slice": lambda: ctx.sort_indices_keys(keys, rows, out),
                    "select_k_radix": lambda: ctx.select_k(keys, rows, k, out, 1),
                    "select_k_sort": lambda: ctx.select_k(keys, rows, k, out, 2),
                }
                times = {name: [] for name in calls}
                for rep in range(args.warmup + args.reps):
                    for name, fn in calls.items():
                        ctx.sync()
                        t0 = time.perf_counter()
                        fn()
                        ctx.sync()   # sort_indices returns with its last passes still in flight
                        ms = (time.perf_counter() - t0) * 1e3
                        if rep >= args.warmup:
                            times[name].append(ms)
                row = {"column": column, "rows_log2": lg, "k": k}
                for name, ts in times.items():
                    row[name] = {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}
                base = row["sort_indices_slice"]
                row["speedup_auto"] = round(base["median_ms"] / row["select_k_auto"]["median_ms"], 2)
                row["auto_not_slower"] = row["select_k_auto"]["median_ms"] <= base["median_ms"] + (base["max_ms"] - base["min_ms"])
                results.append(row)
                print(json.dumps(row), flush=True)
        a.free()
        b.free()
        out.free()
    doc = {"reps": args.reps, "warmup": args.warmup, "unit": "ms per call, host clock, drained stream to drained stream",
           "all_auto_not_slower": all(r["auto_not_slower"] for r in results), "results": results}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    print(json.dumps({"all_auto_not_slower": doc["all_auto_not_slower"], "cases": len(results), "out": args.out}))


if __name__ == "__main__":
    main()
