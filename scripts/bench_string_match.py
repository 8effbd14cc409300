"""The string predicates at 2^24 rows beside ah_compare_binary `equal` against a scalar on the same column, in one process
(DESIGN.md §3.17).

Columns: mean row lengths 8, 32 and 128 bytes (lengths uniform in 0 … 2 · mean; the 128-byte column has 2^31 value bytes and
therefore 8-byte offsets) and one skewed column (mean 8, plus sixteen rows of 8 MiB).  The bytes are the letters a-d; a 16-byte
pattern is planted into half of the rows that can hold it, so "hit" patterns occur in many rows and "miss" patterns (they end in a
letter the column does not have) in none.  Cases per column: match_substring with a missing and a present pattern of 4 and 16
bytes, starts_with, match_like '%a%b%', utf8_length, and `equal` against a scalar — which reads every offset but only the bytes of
the rows as long as the scalar, so it is a floor for a pass over the column, not a pass over the same bytes.

Every call is timed with device events around it (ah_timer_start / _stop), the cases alternating inside each repetition; per case
the median and the spread.  Bytes are what the algorithm must read — the value bytes once and the offsets once, lengths: the offsets
only — computed here from the shapes; rates are those bytes over the time, beside the copy ceiling of the chip (≈ 6.3 TB/s).

    python scripts/bench_string_match.py [--out profiles/string_match_bench.json] [--rows-log2 24] [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah  # noqa: E402
from arrow_go_amd import compute as ac  # noqa: E402

COPY_CEILING_TB_S = 6.3
HIT4, HIT16 = b"abcd", b"abcdabcdabcdabcd"
MISS4, MISS16 = b"abcz", b"abcdabcdabcdabcz"


def make_column(rng, n, mean, skew_rows=0, skew_bytes=0):
    lens = rng.integers(0, 2 * mean + 1, n).astype(np.int64)
    if skew_rows:
        lens[rng.choice(n, skew_rows, replace=False)] = skew_bytes
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    total = int(offsets[-1])
    data = rng.integers(97, 101, total, dtype=np.uint8)
    rows = np.flatnonzero((lens >= 16) & (rng.random(n) < 0.5))
    at = offsets[rows] + (rng.random(len(rows)) * (lens[rows] - 15)).astype(np.int64)
    for k in range(16):
        data[at + k] = HIT16[k]
    ow = 4 if total < 2**31 else 8
    return offsets.astype(np.int32 if ow == 4 else np.int64), data, ow, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "string_match_bench.json"))
    ap.add_argument("--rows-log2", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    n = 1 << args.rows_log2
    rng = np.random.default_rng(17)
    like_program = ac.like_compile("%a%b%")
    doc = {"rows_log2": args.rows_log2, "reps": args.reps, "warmup": args.warmup, "copy_ceiling_tb_per_s": COPY_CEILING_TB_S,
           "unit": "ms per call between device events on the compute stream; the cases alternate inside every repetition",
           "bytes": "value bytes + offsets, each once (lengths and equal: see the script); outputs not counted", "columns": {}}
    with ah.Context(0) as ctx:
        for name, mean, skew in (("mean_8", 8, (0, 0)), ("mean_32", 32, (0, 0)), ("mean_128", 128, (0, 0)), ("skewed_mean_8_plus_16x8MiB", 8, (16, 8 << 20))):
            offsets, data, ow, total = make_column(rng, n, mean, *skew)
            d_off, d_data = ctx.to_device(offsets, pad=8), ctx.to_device(data, pad=16)
            col = (ow, 0, d_off, d_data, 0)
            scalar_offsets = ctx.to_device(np.array([0, len(HIT16)], np.int32 if ow == 4 else np.int64), pad=8)
            scalar_data = ctx.to_device(np.frombuffer(HIT16, np.uint8), pad=16)
            bits, ints = ctx.alloc(n // 8 + 8), ctx.alloc(n * ow)
            read = total + (n + 1) * ow
            cases = {
                "equal_scalar": (lambda: ctx.compare_binary(0, col + (0,), (ow, 0, scalar_offsets, scalar_data, 0, 1), n, bits), read),
                "match_substring_miss_4": (lambda: ctx.string_match(0, col, n, MISS4, bits), read),
                "match_substring_miss_16": (lambda: ctx.string_match(0, col, n, MISS16, bits), read),
                "match_substring_hit_4": (lambda: ctx.string_match(0, col, n, HIT4, bits), read),
                "match_substring_hit_16": (lambda: ctx.string_match(0, col, n, HIT16, bits), read),
                "starts_with_4": (lambda: ctx.string_match(1, col, n, HIT4, bits), (n + 1) * ow),
                "match_like_%a%b%": (lambda: ctx.string_like(col, n, True, like_program, bits), read),
                "utf8_length": (lambda: ctx.string_length(col, n, True, ow, ints), read),
            }
            times = {c: [] for c in cases}
            for rep in range(args.warmup + args.reps):
                for c, (call, _) in cases.items():
                    ctx.timer_start()
                    call()
                    ms = ctx.timer_stop()
                    if rep >= args.warmup:
                        times[c].append(ms)
            results = {}
            for c, ts in times.items():
                med = statistics.median(ts)
                results[c] = {"median_ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "bytes": cases[c][1],
                              "tb_per_s": round(cases[c][1] / med / 1e9, 3), "share_of_copy_ceiling": round(cases[c][1] / med / 1e9 / COPY_CEILING_TB_S, 3)}
            base = results["equal_scalar"]["median_ms"]
            for c in results:
                results[c]["over_equal_scalar"] = round(results[c]["median_ms"] / base, 3)
            doc["columns"][name] = {"value_bytes": total, "offset_width": ow, "results": results}
            del d_off, d_data, bits, ints
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    print(json.dumps({k: {c: r["median_ms"] for c, r in v["results"].items()} for k, v in doc["columns"].items()}))


if __name__ == "__main__":
    main()
