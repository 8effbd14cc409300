"""The typed aggregates over caller-supplied ids (csrc/ah_group_agg.hip) at 2^26 rows and 2^10 groups, ms per call.

  copy    the machine's copy-kernel rate (ah_copy_async of 512 MiB, read + written bytes per second)
  int32   ah_group_sum_typed on an Int32 column against what a caller had to do before it: ah_cast_numeric Int32 -> Int64, then
          ah_group_sum_i64 over the 8-byte copy — both steps in one timed window
  float   the same for Float32: ah_cast_numeric Float32 -> Float64, then ah_group_sum_f64
  count   ah_group_count with and without a validity bitmap, and the fraction of the copy rate its 4 B/row stream reaches

Every figure is the median of ROUNDS windows of CALLS back-to-back calls between two device events, after WARM warm-ups; the rounds
are listed, and "spread" is (max - min) / median over them.
      python scripts/bench_group_agg_typed.py [--rows-log2 26] [--groups-log2 10] [--out profiles/group_agg_typed.json]
"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah
from arrow_go_amd._native import lib, check, INT32, INT64, FLOAT32, FLOAT64

WARM, CALLS, ROUNDS = 2, 3, 7
ap = argparse.ArgumentParser()
ap.add_argument("--rows-log2", type=int, default=26)
ap.add_argument("--groups-log2", type=int, default=10)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_agg_typed.json"))
args = ap.parse_args()
if ah.device_count() < 1:
    raise SystemExit("bench_group_agg_typed: no GPU visible")
ctx = ah.Context(0)
n, ng = 1 << args.rows_log2, 1 << args.groups_log2
chunk = min(n, 1 << 22)
rng = np.random.default_rng(1)


def timed(fn):
    for _ in range(WARM): fn()
    xs = []
    for _ in range(ROUNDS):
        ctx.sync(); ctx.event_record(1)
        for _ in range(CALLS): fn()
        ctx.event_record(2); ctx.sync()
        xs.append(round(ctx.event_elapsed_ms(1, 2) / CALLS, 4))
    med = float(np.median(xs))
    return {"median": round(med, 4), "min": min(xs), "max": max(xs), "spread": round((max(xs) - min(xs)) / med, 4), "rounds": xs}


res = {"what": f"scripts/bench_group_agg_typed.py: 2^{args.rows_log2} rows, 2^{args.groups_log2} groups, ms per call", "warmups": WARM,
       "calls_per_window": CALLS, "rounds": ROUNDS}
nb = 512 << 20
src, dst = ctx.alloc(nb), ctx.alloc(nb)
src.memset(1); dst.memset(2)
t = timed(lambda: check(ctx.handle, lib.ah_copy_async(ctx.handle, dst.ptr, src.ptr, nb)))
copy_rate = 2 * nb / (t["median"] * 1e-3)
res["copy"] = {"bytes": nb, "ms": t, "TB_per_s_read_plus_written": round(copy_rate / 1e12, 3)}
print("copy:", res["copy"]["TB_per_s_read_plus_written"], "TB/s", flush=True)
src.free(); dst.free()

ids, narrow, wide, bits = ctx.alloc(n * 4 + 64), ctx.alloc(n * 4 + 64), ctx.alloc(n * 8 + 64), ctx.alloc(n // 8 + 64)
sums, cnts = ctx.alloc(ng * 8 + 64), ctx.alloc(ng * 8 + 64)
for off in range(0, n, chunk):
    ids.upload(rng.integers(0, ng, chunk).astype(np.int32), off * 4)
    bits.upload(np.packbits(rng.random(chunk) < 0.85, bitorder="little"), off // 8)


def pair(name, in_type, out_type, kind, fill):
    for off in range(0, n, chunk):
        narrow.upload(fill(chunk), off * 4)

    def before():
        ctx.cast_numeric(in_type, out_type, narrow, None, 0, n, False, False, wide)
        ctx.group_sum(kind, ids, ng, wide, None, 0, n, sums, cnts)

    r = {"typed_ms": timed(lambda: ctx.group_sum_typed(in_type, ids, ng, narrow, None, 0, n, sums, cnts)),
         "cast_then_sum_ms": timed(before),
         "cast_alone_ms": timed(lambda: ctx.cast_numeric(in_type, out_type, narrow, None, 0, n, False, False, wide)),
         "sum_over_the_cast_column_alone_ms": timed(lambda: ctx.group_sum(kind, ids, ng, wide, None, 0, n, sums, cnts)),
         "typed_with_validity_ms": timed(lambda: ctx.group_sum_typed(in_type, ids, ng, narrow, bits, 0, n, sums, cnts))}
    r["typed_over_before"] = round(r["typed_ms"]["median"] / r["cast_then_sum_ms"]["median"], 4)
    r["typed_GB_per_s_of_8_B_per_row"] = round(8 * n / (r["typed_ms"]["median"] * 1e-3) / 1e9, 1)
    res[name] = r
    print(name + ":", {k: (v["median"] if isinstance(v, dict) else v) for k, v in r.items()}, flush=True)


pair("int32", INT32, INT64, "i64", lambda m: rng.integers(-2**31, 2**31, m, dtype=np.int64).astype(np.int32))
pair("float32", FLOAT32, FLOAT64, "f64", lambda m: rng.normal(0, 1e3, m).astype(np.float32))

r = {"all_rows_ms": timed(lambda: ctx.group_count(ids, ng, None, 0, n, cnts)),
     "with_validity_ms": timed(lambda: ctx.group_count(ids, ng, bits, 0, n, cnts))}
r["all_rows_GB_per_s_of_4_B_per_row"] = round(4 * n / (r["all_rows_ms"]["median"] * 1e-3) / 1e9, 1)
# the copy kernel moves read + written bytes; a read-only stream is held against the same byte rate
r["fraction_of_the_copy_rate"] = round(4 * n / (r["all_rows_ms"]["median"] * 1e-3) / copy_rate, 3)
res["count"] = r
print("count:", {k: (v["median"] if isinstance(v, dict) else v) for k, v in r.items()}, flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
