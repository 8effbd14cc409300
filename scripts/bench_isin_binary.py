"""is_in by byte-string keys, warm calls on device-resident columns (no upload in the timing), next to Int64 is_in of the same
length:  python scripts/bench_isin_binary.py [lg=24] [reps=5]

  random-16 / -1k / -64k   8-32-byte values of random letters against 16, 1024 and 65 536 entries (LDS, LDS, HBM tiers);
                           half of the set drawn from the column
  category-1k              1000 distinct 10-30-byte names against 1024 entries (the names and 24 others)
  decimal128-1k            random Decimal128 against 1024 entries
  dict-string-1k           the category column dictionary-encoded (int32 indices): is_in of the 1000 entries + the index gather
  int64-1k                 random Int64 against 1024 entries (ah_is_in, the numeric path)
One JSON line per input: {"input", "rows", "set", "ms", "grows_per_s", "data_bytes"}."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah  # noqa: E402

lg = int(sys.argv[1]) if len(sys.argv) > 1 else 24
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rows = 1 << lg
rng = np.random.default_rng(3)
ctx = ah.Context(0)
MATCH = 0


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


def category_names():
    nlen = rng.integers(10, 31, 1000)
    return [rng.integers(97, 123, k, dtype=np.uint8).tobytes() for k in nlen]


def strings_column(words, pick):
    lens = np.array([len(w) for w in words], np.int64)[pick]
    offs = np.zeros(len(pick) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    blob = np.frombuffer(b"".join(words), np.uint8)
    starts = np.concatenate([[0], np.cumsum([len(w) for w in words])[:-1]]).astype(np.int64)
    data = np.empty(int(offs[-1]), np.uint8)
    for lo in range(0, len(pick), 1 << 20):
        hi = min(len(pick), lo + (1 << 20))
        ln = lens[lo:hi]
        rel = np.arange(offs[hi] - offs[lo]) - np.repeat(offs[lo:hi] - offs[lo], ln)
        data[offs[lo]:offs[hi]] = blob[np.repeat(starts[pick[lo:hi]], ln) + rel]
    return offs.astype(np.int32), data


def set_of(words):
    offs = np.zeros(len(words) + 1, np.int64)
    np.cumsum([len(w) for w in words], out=offs[1:])
    return upload(offs.astype(np.int32)), upload(np.frombuffer(b"".join(words) or b"\0", np.uint8))


def timed(fn):
    fn()
    ctx.sync()
    ctx.event_record(10)
    for _ in range(reps):
        fn()
    ctx.event_record(11)
    ctx.sync()
    return ctx.event_elapsed_ms(10, 11) / reps


def report(name, nset, ms, nbytes):
    print(json.dumps({"input": name, "rows": rows, "set": nset, "ms": round(ms, 3), "grows_per_s": round(rows / ms / 1e6, 3),
                      "data_bytes": int(nbytes)}), flush=True)


od, ov = ctx.alloc(rows // 8 + 64), ctx.alloc(rows // 8 + 64)
# random 8-32-byte strings
offs, data = var_column(rng.integers(8, 33, rows), letters)
o, d = upload(offs), upload(data)
for nset in (16, 1024, 65536):
    take = rng.integers(0, rows, nset // 2)
    words = [data[offs[i]:offs[i + 1]].tobytes() for i in take]
    words += [rng.integers(97, 123, 20, dtype=np.uint8).tobytes() for _ in range(nset - len(words))]
    so, sd = set_of(words)
    ms = timed(lambda: ctx.is_in_binary(4, o, d, None, 0, rows, [(4, so, sd, None, 0, nset)], MATCH, od, ov))
    report("random-%s" % ({16: "16", 1024: "1k", 65536: "64k"}[nset]), nset, ms, offs.nbytes + data.nbytes)
del o, d
# category column, plain and dictionary-encoded
names = category_names()
pick = rng.integers(0, 1000, rows)
offs, data = strings_column(names, pick)
o, d = upload(offs), upload(data)
setw = names + [b"other-%d" % i for i in range(24)]
so, sd = set_of(setw)
ms = timed(lambda: ctx.is_in_binary(4, o, d, None, 0, rows, [(4, so, sd, None, 0, len(setw))], MATCH, od, ov))
report("category-1k", len(setw), ms, offs.nbytes + data.nbytes)
del o, d
do, dd = set_of(names)
idx = upload(pick.astype(np.int32))
lut_d, lut_v = ctx.alloc(256), ctx.alloc(256)
null_row = upload(np.zeros(2, np.int32))   # the null value behind the dictionary: offsets (0, 0), validity bit 0
zero = upload(np.zeros(8, np.uint8))


def dict_call():
    ctx.is_in_binary(4, do, dd, None, 0, 1000, [(4, so, sd, None, 0, len(setw))], MATCH, lut_d, lut_v)
    ctx.is_in_binary(4, null_row, zero, zero, 0, 1, [(4, so, sd, None, 0, len(setw))], MATCH, lut_d, lut_v, 1000)
    ctx.is_in_dict_gather(4, idx, None, 0, rows, lut_d, lut_v, 1000, od, ov)


ms = timed(dict_call)
report("dict-string-1k", len(setw), ms, rows * 4)
del idx
# Decimal128
dec = upload(rng.integers(0, 2**63, rows * 2, dtype=np.uint64))
dset = upload(rng.integers(0, 2**63, 1024 * 2, dtype=np.uint64))
ms = timed(lambda: ctx.is_in_fixed(16, dec, None, 0, rows, [(0, None, dset, None, 0, 1024)], MATCH, od, ov))
report("decimal128-1k", 1024, ms, rows * 16)
del dec
ints = upload(rng.integers(-2**62, 2**62, rows, dtype=np.int64))
iset = upload(rng.integers(-2**62, 2**62, 1024, dtype=np.int64))
ms = timed(lambda: ctx.is_in(8, ints, None, 0, rows, iset, None, 0, 1024, MATCH, od, ov))
report("int64-1k", 1024, ms, rows * 8)
