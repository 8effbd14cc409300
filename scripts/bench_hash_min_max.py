"""hash_min_max against the id-based hash_sum (option groupby_partition = 0) of the same kind: 2^26 rows at 2^10 / 2^16 / 2^20 / 2^24 groups,
Int64 and Float64 values.
Both are timed in one process on the same columns, alternating, with device events around `CALLS` back-to-back calls after `WARM`
warm-ups of each; `ROUNDS` rounds give the spread.  Writes profiles/hash_min_max.json (ms per call).

    python scripts/bench_hash_min_max.py [--rows-log2 26] [--out profiles/hash_min_max.json]
"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah

WARM, CALLS, ROUNDS = 2, 4, 5
ap = argparse.ArgumentParser()
ap.add_argument("--rows-log2", type=int, default=26)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hash_min_max.json"))
args = ap.parse_args()
if ah.device_count() < 1:
    raise SystemExit("bench_hash_min_max: no GPU visible")

ctx = ah.Context(0)
ctx.set_option("groupby_partition", 0)   # hash_sum: never the partition-first group-by — the id-based path, which hash_min_max shares up to the aggregate
hrows = 1 << args.rows_log2
chunk = min(hrows, 1 << 22)
rng = np.random.default_rng(1)
keys = ctx.alloc(hrows * 8)
vals = {"i64": ctx.alloc(hrows * 8), "f64": ctx.alloc(hrows * 8)}
for off in range(0, hrows, chunk):
    vals["i64"].upload(rng.integers(-2**62, 2**62, chunk, dtype=np.int64), off * 8)
    vals["f64"].upload(rng.standard_normal(chunk), off * 8)
dic, a, b, cnts = (ctx.alloc((hrows + 1) * 8) for _ in range(4))


def timed(fn):
    for _ in range(WARM): fn()
    ctx.sync(); ctx.event_record(1)
    for _ in range(CALLS): fn()
    ctx.event_record(2); ctx.sync()
    return ctx.event_elapsed_ms(1, 2) / CALLS


res = {"what": f"scripts/bench_hash_min_max.py: 2^{args.rows_log2} rows, ms per call; hash_sum with groupby_partition = 0 (the id-based path)",
       "warmups": WARM, "calls_per_window": CALLS, "rounds": ROUNDS, "results": {}}
for lg in (10, 16, 20, 24):
    if lg > args.rows_log2:
        continue
    card = 1 << lg
    for off in range(0, hrows, chunk):
        keys.upload(rng.integers(0, card, chunk, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15), off * 8)
    for kind in ("i64", "f64"):
        v = vals[kind]
        mm = lambda: ctx.hash_min_max(kind, keys, None, 0, v, None, 0, hrows, dic, a, b, cnts)
        sm = lambda: ctx.hash_sum(kind, keys, None, 0, v, None, 0, hrows, dic, a, cnts)
        t = {"hash_min_max": [], "hash_sum_ids": []}
        for _ in range(ROUNDS):     # alternate, so that a drift of the machine lands on both
            t["hash_min_max"].append(round(timed(mm), 4))
            t["hash_sum_ids"].append(round(timed(sm), 4))
        ng, _ = mm()
        r = {"groups": ng}
        for name, xs in t.items():
            r[name + "_ms"] = {"median": round(float(np.median(xs)), 4), "min": min(xs), "max": max(xs), "rounds": xs}
        r["ratio_of_medians"] = round(r["hash_min_max_ms"]["median"] / r["hash_sum_ids_ms"]["median"], 3)
        res["results"][f"{kind} 2^{lg}"] = r
        print(f"{kind} 2^{lg}: " + "  ".join(f"{name} {r[name + '_ms']['median']:.3f} ms" for name in t), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps({k: (v["hash_min_max_ms"]["median"], v["hash_sum_ids_ms"]["median"]) for k, v in res["results"].items()}))
