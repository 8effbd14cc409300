"""The conditionals at 2^27 Int64 rows beside the Int64 Add of the same process.

if_else of two arrays moves what Add moves — two 8-byte reads and one 8-byte write per row, 24 B — plus one bit per row for the
condition (and three more with validity bitmaps, plus the output's), so Add, measured in the same run on the same buffers, is its
ceiling and the only fair comparison; the ratio is recorded, no figure is fixed.  The directed fill is measured on both routes:
the fused entry (ah_fill_null_directed: 16 B/row + bitmaps) and indices + Take (ah_fill_null_indices writes 4 B/row, which
ah_take_primitive_dev reads again beside the values: 24 B/row + bitmaps).

Every call is timed with device events around it (ah_timer_start / _stop), the cases alternating inside each repetition; per case
the median and the spread.  Rates are the bytes the algorithm needs — computed here from the shapes — over that time.

    python scripts/bench_conditional.py [--out profiles/conditional_bench.json] [--rows-log2 27] [--reps 15] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah  # noqa: E402
from arrow_go_amd import _native as N  # noqa: E402


def bitmap(rng, n, null_rate):
    return np.packbits(rng.random(n) >= null_rate, bitorder="little")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "conditional_bench.json"))
    ap.add_argument("--rows-log2", type=int, default=27)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    n = 1 << args.rows_log2
    nbm = n // 8
    rng = np.random.default_rng(3)
    with ah.Context(0) as ctx:
        a = ctx.to_device(rng.integers(-2**62, 2**62, n, dtype=np.int64))
        b = ctx.to_device(rng.integers(-2**62, 2**62, n, dtype=np.int64))
        out, out2 = ctx.alloc(n * 8), ctx.alloc(n * 8)
        cond = ctx.to_device(bitmap(rng, n, 0.5), pad=8)
        valid = [ctx.to_device(bitmap(rng, n, 0.1), pad=8) for _ in range(3)]   # the condition's, the left side's, the right side's
        out_valid = ctx.alloc(nbm + 8)
        idx, idx_valid, status = ctx.alloc(n * 4), ctx.alloc(nbm + 8), ctx.alloc(16)
        side = lambda buf, v: (0, 8, None, buf, v, 0, 0)
        cases = {
            # name: (call, bytes the algorithm moves)
            "add_int64": (lambda: ctx.arithmetic(N.INT64, N.OP_ADD, N.SHAPE_AA, a, b, out, n), 24 * n),
            "if_else_no_nulls": (lambda: ctx.if_else(cond, None, 0, side(a, None), side(b, None), n, out, None), 24 * n + nbm),
            "if_else_nulls_10pct": (lambda: ctx.if_else(cond, valid[0], 0, side(a, valid[1]), side(b, valid[2]), n, out, out_valid), 24 * n + 5 * nbm),
            "fill_forward_fused": (lambda: ctx.fill_null_directed(8, a, valid[1], 0, n, 0, out, out_valid, want_null_count=False), 16 * n + 2 * nbm),
            "fill_backward_fused": (lambda: ctx.fill_null_directed(8, a, valid[1], 0, n, 1, out, out_valid, want_null_count=False), 16 * n + 2 * nbm),
            "fill_forward_indices_take": (lambda: (ctx.fill_null_indices(valid[1], 0, n, 0, idx, idx_valid, want_null_count=False),
                                                   ctx.take_primitive_dev(8, a, None, 0, n, 4, False, idx, idx_valid, 0, n, out2, out_valid, status)),
                                          24 * n + 4 * nbm),
        }
        times = {name: [] for name in cases}
        for rep in range(args.warmup + args.reps):
            for name, (call, _) in cases.items():
                ctx.timer_start()
                call()
                ms = ctx.timer_stop()
                if rep >= args.warmup:
                    times[name].append(ms)
        # the two fill routes leave the same values
        ctx.fill_null_directed(8, a, valid[1], 0, n, 0, out, out_valid, want_null_count=False)
        cases["fill_forward_indices_take"][0]()
        ctx.sync()
        head = 1 << 20
        assert out.download(np.int64, head).tobytes() == out2.download(np.int64, head).tobytes(), "the two routes of fill_null_forward differ"
    results = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        results[name] = {"median_ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "bytes": cases[name][1],
                         "tb_per_s": round(cases[name][1] / med / 1e9, 3)}
    add = results["add_int64"]["median_ms"]
    ratios = {
        "if_else_no_nulls_over_add": round(results["if_else_no_nulls"]["median_ms"] / add, 4),
        "if_else_nulls_10pct_over_add": round(results["if_else_nulls_10pct"]["median_ms"] / add, 4),
        "fill_forward_indices_take_over_fused": round(results["fill_forward_indices_take"]["median_ms"] / results["fill_forward_fused"]["median_ms"], 4),
    }
    doc = {"rows_log2": args.rows_log2, "type": "int64", "reps": args.reps, "warmup": args.warmup,
           "unit": "ms per call between device events on the compute stream; the cases alternate inside every repetition",
           "nulls": "10 % in the condition and in both sides (if_else_nulls_10pct), 10 % in the filled column; the condition is true for half the rows",
           "results": results, "ratios": ratios}
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    print(json.dumps({"ratios": ratios, "add_tb_per_s": results["add_int64"]["tb_per_s"], "out": args.out}))


if __name__ == "__main__":
    main()
