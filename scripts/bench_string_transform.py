"""The string transforms at 2^24 rows beside the project's existing way to copy a string column — ah_take_binary_offsets +
ah_take_binary_data with identity indices — on the same column, in one process.

Columns: those of scripts/bench_string_match.py — mean row lengths 8, 32 and 128 bytes (lengths uniform in 0 … 2 · mean; the
128-byte column has 2^31 value bytes and therefore 8-byte offsets) and one skewed column (mean 8, plus sixteen rows of 8 MiB).  The
bytes are the letters a-d; every row of 8 bytes or more carries 0-3 spaces at each end.  Cases per column: ascii_upper (the whole
row through the byte map), utf8_slice_codeunits (0, 2), (2, absent) and (-4, absent), ascii_trim_whitespace, utf8_trim of the
code points " a€", and the Take.

The two passes are timed apart, each between device events (ah_timer_start / _stop; the ranges pass ends in its one
synchronisation, which the events include), the cases alternating inside each repetition; per pass the median and the spread.
Bytes per pass are computed here from the shapes: the ranges pass reads the offsets and writes the source starts, the lengths, their
scan and the output offsets (the row bytes a slice or a trim looks at are NOT counted: they depend on the data); the gather reads the
output offsets, the source starts and the kept bytes and writes the kept bytes.

    python scripts/bench_string_transform.py [--out profiles/string_transform_bench.json] [--rows-log2 24] [--reps 10] [--warmup 2]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah  # noqa: E402
from arrow_go_amd import _native as N  # noqa: E402

COPY_CEILING_TB_S = 6.3
UPPER = bytes(c - 32 if 97 <= c <= 122 else c for c in range(256))
WHITESPACE = b"\t\n\v\f\r "


def make_column(rng, n, mean, skew_rows=0, skew_bytes=0):
    lens = rng.integers(0, 2 * mean + 1, n).astype(np.int64)
    if skew_rows:
        lens[rng.choice(n, skew_rows, replace=False)] = skew_bytes
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    total = int(offsets[-1])
    data = rng.integers(97, 101, total, dtype=np.uint8)
    left, right = rng.integers(0, 4, n), rng.integers(0, 4, n)
    for k in range(3):   # 0-3 spaces at each end of the rows that can hold them
        rows = np.flatnonzero((lens >= 8) & (left > k))
        data[offsets[rows] + k] = 32
        rows = np.flatnonzero((lens >= 8) & (right > k))
        data[offsets[rows + 1] - 1 - k] = 32
    ow = 4 if total < 2**31 else 8
    return offsets.astype(np.int32 if ow == 4 else np.int64), data, ow, total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "string_transform_bench.json"))
    ap.add_argument("--rows-log2", type=int, default=24)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    n = 1 << args.rows_log2
    rng = np.random.default_rng(17)
    doc = {"rows_log2": args.rows_log2, "reps": args.reps, "warmup": args.warmup, "copy_ceiling_tb_per_s": COPY_CEILING_TB_S,
           "unit": "ms per pass between device events on the compute stream; the cases alternate inside every repetition",
           "bytes": "per pass, from the shapes (see the script); the row bytes the ranges pass of a slice or a trim looks at are not counted",
           "columns": {}}
    cases = {
        "ascii_upper": (N.STX_WHOLE, {}, UPPER),
        "utf8_slice_codeunits_0_2": (N.STX_SLICE_CODEPOINTS, {"start": 0, "stop": 2}, None),
        "utf8_slice_codeunits_2_end": (N.STX_SLICE_CODEPOINTS, {"start": 2}, None),
        "utf8_slice_codeunits_-4_end": (N.STX_SLICE_CODEPOINTS, {"start": -4}, None),
        "ascii_trim_whitespace": (N.STX_TRIM_BYTES, {"sides": 3, "chars": WHITESPACE}, None),
        "utf8_trim": (N.STX_TRIM_CODEPOINTS, {"sides": 3, "chars": " a€".encode()}, None),
    }
    with ah.Context(0) as ctx:
        for name, mean, skew in (("mean_8", 8, (0, 0)), ("mean_32", 32, (0, 0)), ("mean_128", 128, (0, 0)), ("skewed_mean_8_plus_16x8MiB", 8, (16, 8 << 20))):
            offsets, data, ow, total = make_column(rng, n, mean, *skew)
            d_off, d_data = ctx.to_device(offsets, pad=8), ctx.to_device(data, pad=16)
            col = (ow, 0, d_off, d_data, 0)
            d_idx = ctx.to_device(np.arange(n, dtype=np.uint32))
            starts, out_off, out_data = ctx.alloc(n * ow), ctx.alloc((n + 1) * ow), ctx.alloc(total + 16)
            ranges_bytes = (n + 1) * ow + n * ow + (n + 1) * ow + 32 * n
            times = {c: {"ranges": [], "gather": []} for c in cases}
            times["take_identity"] = {"ranges": [], "gather": []}
            kept = {}
            for rep in range(args.warmup + args.reps):
                for c, (op, kw, byte_map) in cases.items():
                    ctx.timer_start()
                    kept[c] = ctx.string_ranges(op, col, n, starts, out_off, **kw)
                    t_ranges = ctx.timer_stop()
                    ctx.timer_start()
                    ctx.string_gather(col, starts, out_off, n, out_data, byte_map)
                    t_gather = ctx.timer_stop()
                    if rep >= args.warmup:
                        times[c]["ranges"].append(t_ranges)
                        times[c]["gather"].append(t_gather)
                ctx.timer_start()
                _, kept["take_identity"] = ctx.take_binary_offsets(ow, d_off, None, 0, n, 4, False, d_idx, None, 0, n, out_off, None)
                t_ranges = ctx.timer_stop()
                ctx.timer_start()
                ctx.take_binary_data(ow, d_off, d_data, 0, 4, d_idx, n, out_off, out_data)
                t_gather = ctx.timer_stop()
                if rep >= args.warmup:
                    times["take_identity"]["ranges"].append(t_ranges)
                    times["take_identity"]["gather"].append(t_gather)
            results = {}
            for c, ts in times.items():
                gather_bytes = (n + 1) * ow + n * (ow if c != "take_identity" else 4 + ow) + 2 * kept[c]
                first = ranges_bytes if c != "take_identity" else (n + 1) * ow + 4 * n + (n + 1) * ow + 32 * n
                r = {"kept_bytes": kept[c]}
                for which, nbytes in (("ranges", first), ("gather", gather_bytes)):
                    med = statistics.median(ts[which])
                    r[which] = {"median_ms": round(med, 4), "min_ms": round(min(ts[which]), 4), "max_ms": round(max(ts[which]), 4), "bytes": nbytes,
                                "tb_per_s": round(nbytes / med / 1e9, 3)}
                r["total_ms"] = round(r["ranges"]["median_ms"] + r["gather"]["median_ms"], 4)
                r["gather_value_tb_per_s"] = round(2 * kept[c] / r["gather"]["median_ms"] / 1e9, 3)   # kept bytes in and out over the gather's time
                results[c] = r
            base = results["take_identity"]
            for c, r in results.items():
                r["over_take"] = {"ranges": round(r["ranges"]["median_ms"] / base["ranges"]["median_ms"], 3),
                                  "gather": round(r["gather"]["median_ms"] / base["gather"]["median_ms"], 3), "total": round(r["total_ms"] / base["total_ms"], 3)}
            doc["columns"][name] = {"value_bytes": total, "offset_width": ow, "results": results}
            del d_off, d_data, d_idx, starts, out_off, out_data
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1)
    print(json.dumps({k: {c: [r["ranges"]["median_ms"], r["gather"]["median_ms"], r["gather_value_tb_per_s"]] for c, r in v["results"].items()}
                      for k, v in doc["columns"].items()}))


if __name__ == "__main__":
    main()
