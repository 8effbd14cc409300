"""ah_group_m2 beside ah_group_sum_typed on the same ids and column: 2^R rows, Float64 and Int32 values, 10 % nulls,
2^10, 2^16 and 2^20 groups, ms.

ah_group_m2 makes P passes over the column: the sum (Int32: one, the exact integer sum; Float64: two, the scale of every group and
the fixed-point sum), the scale of the squared deviations and their accumulation — P = 3 for Int32, 4 for Float64.  Every pass reads
the bytes the sum's aggregate pass reads (ids, values, validity bits); the last two add two cached gathers per row (the group's mean
and scale).  The yardstick is the sum call of the same run: one aggregate pass for Int32; for Float64 the streaming absmax pass (no
ids) and one aggregate pass (above 4096 groups the partitioned route of ah_hash_agg.hip).  Reported per shape:
  m2 / sum              device time of ah_group_m2 over device time of ah_group_sum_typed, to be read beside P over the sum's passes
  *_call_ms             host clock around the call and a synchronisation
Device times are medians of ROUNDS windows between two device events after WARM warm-ups; "spread" is (max - min) / median.  The
result of every shape is checked against tests/group_variance_model.py on a sample of groups before anything is timed.
With --once every call runs once after one warm-up and nothing is written: the form to put under a kernel trace, which gives the
passes one by one:
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o var -- python scripts/bench_group_variance.py --once --groups-log2 10
--summarise-trace DIR/var_kernel_stats.csv (needs no GPU) turns that trace into profiles/group_variance_passes.json: every pass of the
two calls in microseconds and, per type, t(m2) / t(sum's aggregate pass) — the passes of ah_group_m2 added up, over the one pass of
the sum call that reads ids and values — beside P.
      python scripts/bench_group_variance.py [--rows-log2 26] [--out profiles/group_variance_bench.json] [--groups-log2 10,16,20] [--once]
      python scripts/bench_group_variance.py --summarise-trace DIR/var_kernel_stats.csv [--passes-out profiles/group_variance_passes.json]
"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, ROUNDS = 2, 7
ap = argparse.ArgumentParser()
ap.add_argument("--rows-log2", type=int, default=26)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_variance_bench.json"))
ap.add_argument("--groups-log2", default="10,16,20")
ap.add_argument("--once", action="store_true")
ap.add_argument("--summarise-trace", default=None)
ap.add_argument("--passes-out", default=os.path.join(ROOT, "profiles", "group_variance_passes.json"))
args = ap.parse_args()
PASSES = {"float64": {"m2": 4, "sum": 2}, "int32": {"m2": 3, "sum": 1}}


def summarise_trace(path, out_path):
    """kernel statistics of a --once run at one group count -> the passes of both calls per type, and t(m2) / t(sum's aggregate pass)"""
    import csv
    kernels = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
        if any(k in name for k in ("agg_kernel", "absmax_kernel", "fx_finalize_kernel", "group_mean_kernel")):
            kernels[name] = {"calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 1), "min_us": round(int(r["MinNs"]) / 1e3, 1),
                             "max_us": round(int(r["MaxNs"]) / 1e3, 1)}
    us = lambda name: kernels[name]["average_us"]   # noqa: E731
    # the aggregate pass of the sum call, and the passes of ah_group_m2 in the order they run (the first of Int32 is the sum's own kernel)
    shape = {"int32": ("typed_agg_kernel<WidenedSumInt, int, true>",
                       ["typed_agg_kernel<WidenedSumInt, int, true>", "cast_agg_kernel<GroupScale<true>, int, true>", "cast_agg_kernel<ScaledSum<true>, int, true>"]),
             "float64": ("group_agg_kernel<SumF64, true>",
                         ["cast_agg_kernel<GroupScale<false>, double, true>", "cast_agg_kernel<ScaledSum<false>, double, true>",
                          "cast_agg_kernel<GroupScale<true>, double, true>", "cast_agg_kernel<ScaledSum<true>, double, true>"])}
    ratios = {}
    for name, (agg, passes) in shape.items():
        assert len(passes) == PASSES[name]["m2"]
        total = sum(us(p) for p in passes)
        ratios[name] = {"sum_aggregate_pass_us": us(agg), "m2_passes_us": [us(p) for p in passes], "m2_passes_total_us": round(total, 1),
                        "m2_over_sum_aggregate_pass": round(total / us(agg), 2), "P": PASSES[name]["m2"]}
    res = {"what": "kernel trace (--kernel-trace --stats, a run of its own) of scripts/bench_group_variance.py --once at one group count: one warm-up "
                   "and one call of ah_group_sum_typed and ah_group_m2 per type, 10 % nulls; per kernel over its calls, microseconds; summarised by "
                   "scripts/bench_group_variance.py --summarise-trace", "ratios": ratios, "kernels": kernels}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(ratios, indent=1))


if args.summarise_trace:
    summarise_trace(args.summarise_trace, args.passes_out)
    raise SystemExit(0)
import arrow_go_amd as ah   # noqa: E402
from tests import group_variance_model as M   # noqa: E402
if ah.device_count() < 1:
    raise SystemExit("bench_group_variance: no GPU visible")
ctx = ah.Context(0)
n = 1 << args.rows_log2
rng = np.random.default_rng(1)
TYPE_IDS = {"float64": 12, "int32": 7}


def timed(fn):
    for _ in range(WARM): fn()
    xs, walls = [], []
    for _ in range(ROUNDS):
        ctx.sync(); ctx.event_record(1)
        t0 = time.perf_counter()
        fn()
        ctx.event_record(2); ctx.sync()
        walls.append(round((time.perf_counter() - t0) * 1e3, 4))
        xs.append(round(ctx.event_elapsed_ms(1, 2), 4))
    med = float(np.median(xs))
    return {"median": round(med, 4), "min": min(xs), "max": max(xs), "spread": round((max(xs) - min(xs)) / med, 4), "rounds": xs,
            "call_ms": round(float(np.median(walls)), 4)}


res = {"what": f"scripts/bench_group_variance.py: ah_group_m2 beside ah_group_sum_typed, 2^{args.rows_log2} rows, 10 % nulls, ms", "warmups": WARM,
       "rounds": ROUNDS, "passes": PASSES, "shapes": {}}
valid = rng.random(n) >= 0.1
bits = ctx.to_device(np.packbits(valid, bitorder="little"), 64)
columns = {"float64": rng.normal(0, 1e3, n), "int32": rng.integers(-10**6, 10**6, n).astype(np.int32)}
for ng_log2 in [int(x) for x in args.groups_log2.split(",")]:
    ng = 1 << ng_log2
    ids_h = rng.integers(0, ng, n).astype(np.int32)
    ids = ctx.to_device(ids_h, 64)
    for name, col in columns.items():
        tid = TYPE_IDS[name]
        vals = ctx.to_device(col, 64)
        means, m2, counts, sums = (ctx.alloc(ng * 8 + 64) for _ in range(4))
        run_m2 = lambda: ctx.group_m2(tid, ids, ng, vals, bits, 0, n, means, m2, counts)   # noqa: E731
        run_sum = lambda: ctx.group_sum_typed(tid, ids, ng, vals, bits, 0, n, sums, counts)   # noqa: E731
        run_m2(); ctx.sync()
        # a sample of groups against the model, before anything is timed
        sample = rng.choice(ng, 6, replace=False)
        got_n, got_m, got_m2 = counts.download(np.int64, ng), means.download(np.float64, ng), m2.download(np.float64, ng)
        for g in sample:
            rows = np.flatnonzero((ids_h == g) & valid)
            c, m, s2 = M.moments(col[rows], np.zeros(len(rows), np.int32), 1)
            assert got_n[g] == c[0] and got_m[g] == m[0] and abs(got_m2[g] - s2[0]) <= np.spacing(s2[0]), (name, ng, int(g))
        if args.once:
            run_sum(); ctx.sync(); run_sum(); run_m2(); ctx.sync()
        else:
            out = {"groups": ng, "rows": n, "sum": timed(run_sum), "m2": timed(run_m2)}
            out["m2_over_sum"] = round(out["m2"]["median"] / out["sum"]["median"], 3)
            out["passes_m2_over_passes_sum"] = round(PASSES[name]["m2"] / PASSES[name]["sum"], 3)
            res["shapes"][f"{name}_2^{ng_log2}"] = out
            print(name, ng, json.dumps({k: (v["median"] if isinstance(v, dict) else v) for k, v in out.items()}), flush=True)
        for b in (vals, means, m2, counts, sums):
            b.free()
    ids.free()
if not args.once:
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({k: v["m2_over_sum"] for k, v in res["shapes"].items()}))
