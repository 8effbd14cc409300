"""Decimal cast throughput at 2^26 rows: the three entry points of ah_cast_decimal.hip against two yardsticks timed
in the same process — a device-to-device hipMemcpyAsync of the same byte volume and ah_cast_numeric int64 → double.

Per case: 3 warm-up calls, then 25 repetitions each between its own pair of events; the median is reported.  Algorithmic bytes per
row: input width + output width.  Usage: python scripts/bench_cast_decimal.py [--rows N] [--out profiles/cast_decimal.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 26)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cast_decimal.json"))
args = ap.parse_args()
rows = args.rows
N = ah._native
WARM, REPS = 3, 25
ctx = ah.Context(0)

# values of at most 15 digits: every safe case below passes its checks (÷ 100 is exact: the low two digits are zero)
rng = np.random.default_rng(0)
v = rng.integers(-10 ** 13, 10 ** 13, rows, dtype=np.int64) * 100
d_i64 = ctx.to_device(v)
d128 = ctx.alloc(rows * 16)
d256 = ctx.alloc(rows * 32)
out = ctx.alloc(rows * 32)
ctx.cast_int_to_decimal(N.INT64, 16, 0, d_i64, None, 0, rows, d128)
ctx.cast_int_to_decimal(N.INT64, 32, 0, d_i64, None, 0, rows, d256)
ctx.sync()


def timed(fn):
    for _ in range(WARM):
        fn()
    ctx.sync()
    for r in range(REPS):
        ctx.event_record(100 + 2 * r)
        fn()
        ctx.event_record(101 + 2 * r)
    ctx.sync()
    return statistics.median(ctx.event_elapsed_ms(100 + 2 * r, 101 + 2 * r) for r in range(REPS))


# the raw runtime copy, on the null stream with events of its own
hip = ctypes.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]


def hip_ok(rc):
    if rc != 0:
        raise RuntimeError("hip call failed: %d" % rc)


def timed_memcpy(nbytes):
    """device-to-device hipMemcpyAsync of nbytes (read nbytes, write nbytes)"""
    ev = [ctypes.c_void_p() for _ in range(2 * REPS)]
    for e in ev:
        hip_ok(hip.hipEventCreate(ctypes.byref(e)))
    src, dst = ah.device._ptr(d256), ah.device._ptr(out)
    for _ in range(WARM):
        hip_ok(hip.hipMemcpyAsync(dst, src, nbytes, 3, None))
    for r in range(REPS):
        hip_ok(hip.hipEventRecord(ev[2 * r], None))
        hip_ok(hip.hipMemcpyAsync(dst, src, nbytes, 3, None))
        hip_ok(hip.hipEventRecord(ev[2 * r + 1], None))
    hip_ok(hip.hipEventSynchronize(ev[-1]))
    ms = []
    for r in range(REPS):
        f = ctypes.c_float()
        hip_ok(hip.hipEventElapsedTime(ctypes.byref(f), ev[2 * r], ev[2 * r + 1]))
        ms.append(f.value)
    return statistics.median(ms)


res = {"rows": rows, "warmup": WARM, "repetitions": REPS, "statistic": "median of per-repetition event pairs", "cases": {}}
copy_ms = {nb: timed_memcpy(rows * nb) for nb in (8, 16, 32)}      # a copy of nb bytes per row moves 2·nb
for nb, ms in copy_ms.items():
    res["cases"]["hipMemcpyAsync D2D %d B/row" % nb] = {"ms": round(ms, 4), "bytes_per_row": 2 * nb, "GBps": round(2 * nb * rows / ms / 1e6)}
copy_rate = max(2 * nb * rows / ms for nb, ms in copy_ms.items())   # bytes per ms of the best copy of this run


def report(name, ms, bytes_per_row):
    rate = bytes_per_row * rows / ms
    res["cases"][name] = {"ms": round(ms, 4), "bytes_per_row": bytes_per_row, "GBps": round(rate / 1e6), "fraction_of_copy": round(rate / copy_rate, 3)}


report("ah_cast_numeric int64 -> double", timed(lambda: ctx.cast_numeric(N.INT64, N.FLOAT64, d_i64, None, 0, rows, False, False, out)), 16)
for name, k, safe in (("d128 -> d128 k=0 unchecked (copy)", 0, False), ("d128 -> d128 k=0 safe", 0, True), ("d128 -> d128 k=+2 safe", 2, True),
                      ("d128 -> d128 k=+2 unchecked", 2, False), ("d128 -> d128 k=+20 safe", 20, True), ("d128 -> d128 k=-2 safe", -2, True),
                      ("d128 -> d128 k=-2 truncating", -2, False)):
    report(name, timed(lambda: ctx.cast_decimal_rescale(16, 16, k, 38, not safe, d128, None, 0, rows, out)), 32)
report("d128 -> d256 k=0 safe", timed(lambda: ctx.cast_decimal_rescale(16, 32, 0, 76, False, d128, None, 0, rows, out)), 48)
report("d128 -> d256 k=0 unchecked (widen)", timed(lambda: ctx.cast_decimal_rescale(16, 32, 0, 76, True, d128, None, 0, rows, out)), 48)
report("d256 -> d256 k=+40 safe", timed(lambda: ctx.cast_decimal_rescale(32, 32, 40, 76, False, d256, None, 0, rows, out)), 64)
# ÷ 10^40 of 15-digit values: not exact, so the safe cast would (rightly) fail — the truncating one is timed
report("d256 -> d256 k=-40 truncating", timed(lambda: ctx.cast_decimal_rescale(32, 32, -40, 76, True, d256, None, 0, rows, out)), 64)
report("d256 -> d256 k=-2 safe", timed(lambda: ctx.cast_decimal_rescale(32, 32, -2, 76, False, d256, None, 0, rows, out)), 64)
report("int64 -> d128 scale 2", timed(lambda: ctx.cast_int_to_decimal(N.INT64, 16, 2, d_i64, None, 0, rows, out)), 24)
report("d128 (scale 2) -> int64 safe", timed(lambda: ctx.cast_decimal_to_int(16, 2, N.INT64, False, False, d128, None, 0, rows, out)), 24)
report("d128 (scale 2) -> int64 truncating", timed(lambda: ctx.cast_decimal_to_int(16, 2, N.INT64, True, False, d128, None, 0, rows, out)), 24)
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(res, open(args.out, "w"), indent=1)
