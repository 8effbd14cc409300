"""Comparisons of byte-string and decimal columns, warm calls on device-resident columns (no upload in the timing), next to
Int64 equal and a 16-entry is_in of the same string column:  python scripts/bench_compare_binary.py [lg=24] [reps=10]

  str8-32 eq/less scalar   random 8-32-byte letter strings against one of its own values (ah_compare_binary, broadcast side)
  str8-32 eq/less array    the same column against a second column of the same kind
  url less array           75-byte URL-like strings that share a 65-byte prefix, against a second such column
  fsb16 less array         FixedSizeBinary(16) against FixedSizeBinary(16)
  decimal128 less array    Decimal128 against Decimal128 (no rescale) and against a side rescaled by 10^2
  int64 eq array           ah_comparison on Int64 columns
  str8-32 is_in 16         ah_is_in_binary of the string column against 16 of its values
One JSON line per input: {"input", "rows", "ms", "grows_per_s", "touched_bytes", "gbytes_per_s"}.  touched_bytes counts what the
kernel reads and writes: offsets, the 8-byte words it compares up to the first difference (counted on a 64 K-row sample and
scaled; equal / not_equal read no byte of a row whose lengths differ), fixed-width slots, and the output bitmap."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah  # noqa: E402
from arrow_go_amd import _native as N  # noqa: E402

lg = int(sys.argv[1]) if len(sys.argv) > 1 else 24
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
rows = 1 << lg
rng = np.random.default_rng(5)
ctx = ah.Context(0)
EQ, NE, GT, GE = N.CMP_EQ, N.CMP_NE, N.CMP_GT, N.CMP_GE


def upload(arr: np.ndarray):
    raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    buf = ctx.alloc(max(raw.nbytes, 8))
    step = 1 << 28
    for off in range(0, raw.nbytes, step):
        buf.upload(raw[off:off + step], off)
    return buf


def letters_column():
    lens = rng.integers(8, 33, rows)
    offs = np.zeros(rows + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    return offs.astype(np.int32), rng.integers(97, 123, int(offs[-1]), dtype=np.uint8)


def url_column():
    prefix = np.frombuffer(b"https://www.example-cdn-host.com/assets/static/v2/images/product/", np.uint8)  # 65 bytes
    width = len(prefix) + 10
    data = np.empty((rows, width), np.uint8)
    data[:, :len(prefix)] = prefix
    for lo in range(0, rows, 1 << 20):
        ids = rng.integers(0, 10**10, min(rows - lo, 1 << 20))
        data[lo:lo + len(ids), len(prefix):] = (ids[:, None] // 10 ** np.arange(9, -1, -1)) % 10 + 48
    return (np.arange(rows + 1, dtype=np.int64) * width).astype(np.int32), data.reshape(-1)


def value(col, i):
    offs, data = col
    return data[offs[i]:offs[i + 1]].tobytes()


def words_read(a: bytes, b: bytes, eq_op: bool) -> int:
    """bytes one side of the kernel reads for one row: 8-byte words up to the first that differs, capped at the common length"""
    if eq_op and len(a) != len(b):
        return 0
    m = min(len(a), len(b))
    j = 0
    while j < m:
        if a[j:j + 8] != b[j:j + 8]:
            return min(j + 8, m)
        j += 8
    return m


def touched(colA, colB_or_scalar, eq_op, sample=1 << 16):
    """offsets + sampled compared bytes (both sides; a broadcast side is read from LDS and not counted) + the output bitmap"""
    idx = rng.integers(0, rows, sample)
    is_scalar = isinstance(colB_or_scalar, bytes)
    per_row = 0
    for i in idx:
        b = colB_or_scalar if is_scalar else value(colB_or_scalar, i)
        per_row += words_read(value(colA, i), b, eq_op) * (1 if is_scalar else 2)
    offsets = 8 * rows * (1 if is_scalar else 2)  # two 4-byte offsets per row and side
    return int(offsets + per_row / sample * rows + rows / 8)


def timed(fn):
    fn()
    ctx.sync()
    ctx.event_record(10)
    for _ in range(reps):
        fn()
    ctx.event_record(11)
    ctx.sync()
    return ctx.event_elapsed_ms(10, 11) / reps


def report(name, ms, nbytes):
    print(json.dumps({"input": name, "rows": rows, "ms": round(ms, 4), "grows_per_s": round(rows / ms / 1e6, 3), "touched_bytes": int(nbytes),
                      "gbytes_per_s": round(nbytes / ms / 1e6, 1)}), flush=True)


out = ctx.alloc(rows // 8 + 64)
A, B = letters_column(), letters_column()
a_o, a_d, b_o, b_d = upload(A[0]), upload(A[1]), upload(B[0]), upload(B[1])
s_val = value(A, 12345)
s_o, s_d = upload(np.array([0, len(s_val)], np.int32)), upload(np.frombuffer(s_val, np.uint8))
colA = (4, 0, a_o, a_d, 0, 0)
colB = (4, 0, b_o, b_d, 0, 0)
scal = (4, 0, s_o, s_d, 0, 1)
for op, nm, eq in ((EQ, "eq", True), (GT, "less", False)):  # less(a, s) = greater(s, a)
    lhs, rhs = (colA, scal) if op == EQ else (scal, colA)
    report("str8-32 %s scalar" % nm, timed(lambda: ctx.compare_binary(op, lhs, rhs, rows, out)), touched(A, s_val, eq))
for op, nm, eq in ((EQ, "eq", True), (GT, "less", False)):
    lhs, rhs = (colA, colB) if op == EQ else (colB, colA)
    report("str8-32 %s array" % nm, timed(lambda: ctx.compare_binary(op, lhs, rhs, rows, out)), touched(A, B, eq))
# reference points on the same string column: Int64 equal, is_in with 16 entries
ints_a = upload(rng.integers(-2**62, 2**62, rows, dtype=np.int64))
ints_b = upload(rng.integers(-2**62, 2**62, rows, dtype=np.int64))
report("int64 eq array", timed(lambda: ctx.comparison(EQ, N.SHAPE_AA, N.INT64, ints_a, ints_b, out, rows)), rows * 16 + rows / 8)
del ints_a, ints_b
words = [value(A, int(i)) for i in rng.integers(0, rows, 8)] + [rng.integers(97, 123, 20, dtype=np.uint8).tobytes() for _ in range(8)]
so_h = np.zeros(17, np.int32)
so_h[1:] = np.cumsum([len(w) for w in words])
so, sd = upload(so_h), upload(np.frombuffer(b"".join(words), np.uint8))
ov = ctx.alloc(rows // 8 + 64)
report("str8-32 is_in 16", timed(lambda: ctx.is_in_binary(4, a_o, a_d, None, 0, rows, [(4, so, sd, None, 0, 16)], 0, out, ov)),
       A[0].nbytes + A[1].nbytes + rows / 4)
del a_o, a_d, b_o, b_d
U, V = url_column(), url_column()
u_o, u_d, v_o, v_d = upload(U[0]), upload(U[1]), upload(V[0]), upload(V[1])
report("url less array", timed(lambda: ctx.compare_binary(GT, (4, 0, v_o, v_d, 0, 0), (4, 0, u_o, u_d, 0, 0), rows, out)), touched(U, V, False))
del u_o, u_d, v_o, v_d
f_a = upload(rng.integers(97, 123, rows * 16, dtype=np.uint8))
f_b = upload(rng.integers(97, 123, rows * 16, dtype=np.uint8))
report("fsb16 less array", timed(lambda: ctx.compare_binary(GT, (0, 16, None, f_b, 0, 0), (0, 16, None, f_a, 0, 0), rows, out)), rows * 32 + rows / 8)
del f_a, f_b
d_a = upload(rng.integers(-2**62, 2**62, rows * 2, dtype=np.int64))
d_b = upload(rng.integers(-2**62, 2**62, rows * 2, dtype=np.int64))
report("decimal128 less array", timed(lambda: ctx.compare_decimal(GT, (16, d_b, 0, 0, 0), (16, d_a, 0, 0, 0), rows, out)), rows * 32 + rows / 8)
report("decimal128 less array rescaled", timed(lambda: ctx.compare_decimal(GT, (16, d_b, 0, 0, 2), (16, d_a, 0, 0, 0), rows, out)),
       rows * 32 + rows / 8)
