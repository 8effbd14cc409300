"""String cast throughput at 2^24 rows: the entry points of ah_cast_string.hip, device-resident columns, beside a
device-to-device hipMemcpyAsync timed in the same process.

Per case: 3 warm-up calls, then 15 repetitions each between its own pair of events; the median is reported.  The parse, validate and
format-offsets calls return a host value, so their time includes that one synchronisation.  bytes_per_row is the algorithmic traffic
of the call: what it must read and write once (values, offsets, characters), not the temporaries of the scan.
Usage: python scripts/bench_cast_string.py [--rows N] [--out profiles/cast_string.json]"""
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
ap.add_argument("--rows", type=int, default=1 << 24)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cast_string.json"))
args = ap.parse_args()
rows = args.rows
N = ah._native
WARM, REPS = 3, 15
ctx = ah.Context(0)
rng = np.random.default_rng(0)


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


hip = ctypes.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]


def hip_ok(rc):
    if rc != 0:
        raise RuntimeError("hip call failed: %d" % rc)


def timed_memcpy(src, dst, nbytes):
    ev = [ctypes.c_void_p() for _ in range(2 * REPS)]
    for e in ev:
        hip_ok(hip.hipEventCreate(ctypes.byref(e)))
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
a, b = ctx.alloc(rows * 32), ctx.alloc(rows * 32)
copy_ms = timed_memcpy(ah.device._ptr(a), ah.device._ptr(b), rows * 32)
copy_rate = 2 * rows * 32 / copy_ms
res["cases"]["hipMemcpyAsync D2D 32 B/row"] = {"ms": round(copy_ms, 4), "bytes_per_row": 64, "GBps": round(copy_rate / 1e6)}
del a, b


def report(name, ms, bytes_per_row):
    rate = bytes_per_row * rows / ms
    res["cases"][name] = {"ms": round(ms, 4), "bytes_per_row": round(bytes_per_row, 2), "GBps": round(rate / 1e6, 1), "Mrows_per_s": round(rows / ms / 1e3),
                          "fraction_of_copy": round(rate / copy_rate, 3)}


for label, values in (("uniform 64-bit", rng.integers(-2 ** 63, 2 ** 63 - 1, rows, dtype=np.int64)), ("values < 10^5", rng.integers(0, 10 ** 5, rows, dtype=np.int64))):
    d_vals = ctx.to_device(values)
    offs = ctx.alloc((rows + 1) * 4)
    total = ctx.format_int_offsets(N.INT64, d_vals, None, 0, rows, 4, offs)
    chars = total / rows
    data = ctx.alloc(total + 16)
    report("int64 -> string offsets, " + label, timed(lambda: ctx.format_int_offsets(N.INT64, d_vals, None, 0, rows, 4, offs)), 8 + 4)
    report("int64 -> string data, " + label, timed(lambda: ctx.format_int_data(N.INT64, d_vals, None, 0, rows, 4, offs, data)), 8 + 4 + chars)
    out = ctx.alloc(rows * 8)
    report("string -> int64, " + label, timed(lambda: ctx.parse_int(4, offs, data, None, 0, rows, N.INT64, out)), 4 + chars + 8)
    assert np.array_equal(out.download(np.int64, rows), values)
    del d_vals, offs, data, out

bits = ctx.to_device(rng.integers(0, 256, rows // 8 + 8, dtype=np.uint8))
offs = ctx.alloc((rows + 1) * 4)
total = ctx.format_int_offsets(1, bits, None, 0, rows, 4, offs)
data = ctx.alloc(total + 16)
report("boolean -> string offsets", timed(lambda: ctx.format_int_offsets(1, bits, None, 0, rows, 4, offs)), 0.125 + 4)
report("boolean -> string data", timed(lambda: ctx.format_int_data(1, bits, None, 0, rows, 4, offs, data)), 0.125 + 4 + total / rows)
del bits, offs, data


def text_column(multibyte_share):
    """rows of 8 – 32 bytes of valid text: a (1 byte), é (2), 世 (3), cut at character boundaries"""
    nchars = rng.integers(6, 17, rows)
    total_chars = int(nchars.sum())
    w = np.ones(total_chars, np.int64)
    pick = rng.random(total_chars)
    w[pick < multibyte_share / 2] = 2
    w[(pick >= multibyte_share / 2) & (pick < multibyte_share)] = 3
    starts = np.concatenate([[0], np.cumsum(w)])
    data = np.full(int(starts[-1]) + 8, ord("a"), np.uint8)
    s2, s3 = starts[:-1][w == 2], starts[:-1][w == 3]
    data[s2], data[s2 + 1] = 0xC3, 0xA9
    data[s3], data[s3 + 1], data[s3 + 2] = 0xE4, 0xB8, 0x96
    offsets = starts[np.concatenate([[0], np.cumsum(nchars)])].astype(np.int32)
    return ctx.to_device(offsets), ctx.to_device(data), float(starts[-1]) / rows


for label, share in (("ASCII", 0.0), ("30 % multi-byte", 0.3)):
    offs, data, avg = text_column(share)
    report("binary -> string validation, " + label, timed(lambda: ctx.validate_utf8(4, offs, data, 0, None, 0, rows)), 4 + avg)
    del offs, data

print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(res, open(args.out, "w"), indent=1)
