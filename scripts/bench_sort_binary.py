"""sort_indices by binary keys, warm calls on device-resident columns (no upload in the timing), next to an Int64 column of the
same length:  python scripts/bench_sort_binary.py [lg=24] [reps=5]

  random    8-32-byte values of random letters: almost every row is decided by round 0 (the first 7 bytes)
  urls      "https://…/" with a 65-byte shared prefix and a 10-digit id: every row tied for 9 rounds, then decided
  category  1000 distinct 10-30-byte names: 1000 runs of ≈ n / 1000 rows carried through every round of the longest name
  int64     random Int64 (ah_sort_indices, the numeric path)
One JSON line per input: {"input", "rows", "ms", "grows_per_s", "data_bytes"}."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah  # noqa: E402

N = ah._native
AH_BINARY = 14
lg = int(sys.argv[1]) if len(sys.argv) > 1 else 24
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rows = 1 << lg
rng = np.random.default_rng(3)
ctx = ah.Context(0)


def upload(arr: np.ndarray):
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = ctx.alloc(max(raw.nbytes, 8))
    step = 1 << 28
    for off in range(0, raw.nbytes, step):
        buf.upload(raw[off:off + step], off)
    return buf


def var_column(lengths: np.ndarray, fill):
    """offsets (int32) and data of rows whose bytes fill(total_bytes, offsets) produces"""
    offs = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=offs[1:])
    assert offs[-1] < 2**31
    return offs.astype(np.int32), fill(int(offs[-1]), offs)


def letters(total, offs):
    return rng.integers(97, 123, total, dtype=np.uint8)


def urls():
    prefix = np.frombuffer(b"https://www.example-cdn-host.com/assets/static/v2/images/product/", np.uint8)  # 65 bytes
    width = len(prefix) + 10
    data = np.empty((rows, width), np.uint8)
    data[:, :len(prefix)] = prefix
    for lo in range(0, rows, 1 << 20):
        ids = rng.integers(0, 10**10, min(rows - lo, 1 << 20))
        data[lo:lo + len(ids), len(prefix):] = (ids[:, None] // 10 ** np.arange(9, -1, -1)) % 10 + 48
    return (np.arange(rows + 1, dtype=np.int64) * width).astype(np.int32), data.reshape(-1)


def category():
    nlen = rng.integers(10, 31, 1000)
    blob = np.frombuffer(b"".join(rng.integers(97, 123, k, dtype=np.uint8).tobytes() for k in nlen), np.uint8)
    starts = np.concatenate([[0], np.cumsum(nlen)[:-1]])
    pick = rng.integers(0, 1000, rows)
    offs = np.zeros(rows + 1, np.int64)
    np.cumsum(nlen[pick], out=offs[1:])
    data = np.empty(int(offs[-1]), np.uint8)
    for lo in range(0, rows, 1 << 20):  # row i's bytes = blob[starts[pick[i]] : + nlen[pick[i]]]
        hi = min(rows, lo + (1 << 20))
        lens = nlen[pick[lo:hi]]
        rel = np.arange(offs[hi] - offs[lo]) - np.repeat(offs[lo:hi] - offs[lo], lens)
        data[offs[lo]:offs[hi]] = blob[np.repeat(starts[pick[lo:hi]], lens) + rel]
    return offs.astype(np.int32), data


def timed(fn):
    fn()
    ctx.sync()
    ctx.event_record(10)
    for _ in range(reps):
        fn()
    ctx.event_record(11)
    ctx.sync()
    return ctx.event_elapsed_ms(10, 11) / reps


out = ctx.alloc(rows * 8)
inputs = {
    "random": lambda: var_column(rng.integers(8, 33, rows), letters),
    "urls": urls,
    "category": category,
}
for name, make in inputs.items():
    offs, data = make()
    o, d = upload(offs), upload(data)
    ms = timed(lambda: ctx.sort_indices_keys([(AH_BINARY, d, o, 0, None, 0, False, False)], rows, out))
    print(json.dumps({"input": name, "rows": rows, "ms": round(ms, 3), "grows_per_s": round(rows / ms / 1e6, 3), "data_bytes": int(data.nbytes)}),
          flush=True)
    del o, d
ints = upload(rng.integers(-2**62, 2**62, rows, dtype=np.int64))
ms = timed(lambda: ctx.sort_indices(N.INT64, ints, None, 0, rows, False, False, out))
print(json.dumps({"input": "int64", "rows": rows, "ms": round(ms, 3), "grows_per_s": round(rows / ms / 1e6, 3), "data_bytes": rows * 8}), flush=True)
