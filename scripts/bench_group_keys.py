"""ah_group_ids and the aggregates over caller-supplied ids at 2^26 rows, ms per call.

  copy   the machine's copy-kernel rate (ah_copy_async of 512 MiB, read + written bytes per second)
  a      (Int32, Int32) -> ids + Int64 sum at 2^10 / 2^16 / 2^20 groups, against ah_hash_sum_i64 on the same tuples packed into one
         uint64 column on the host (what a caller had to do before ah_group_ids).  ids over the host-packed column (the same
         encoder, no pack pass) and ah_hash_sum_i64 with groupby_partition = 0 (ids + aggregate, no fused partition-first route) are
         timed as well, so that the pack pass and the loss of the fused route can be told apart.
  b      a String key of 8 ... 24 bytes, 2^16 distinct values: ah_group_ids against ah_hash_binary_encode (the same path), then the
         (String, Int32) tuple with the Int32 column a function of the string (the same 2^16 groups: what the tuple policy costs).

Every figure is the median of ROUNDS windows of CALLS back-to-back calls between two device events, after WARM warm-ups; the rounds
are listed.      python scripts/bench_group_keys.py [--rows-log2 26] [--only copy,a,b] [--out profiles/group_keys.json]
"""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah
from arrow_go_amd._native import lib, check

WARM, CALLS, ROUNDS = 1, 3, 5
ap = argparse.ArgumentParser()
ap.add_argument("--rows-log2", type=int, default=26)
ap.add_argument("--only", default="copy,a,b")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_keys.json"))
args = ap.parse_args()
if ah.device_count() < 1:
    raise SystemExit("bench_group_keys: no GPU visible")
ctx = ah.Context(0)
n = 1 << args.rows_log2
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
    return {"median": round(float(np.median(xs)), 4), "min": min(xs), "max": max(xs), "rounds": xs}


res = {"what": f"scripts/bench_group_keys.py: 2^{args.rows_log2} rows, ms per call", "warmups": WARM, "calls_per_window": CALLS, "rounds": ROUNDS}
ids, first = ctx.alloc(n * 4 + 64), ctx.alloc((n + 1) * 8 + 64)

if "copy" in args.only:
    nb = 512 << 20
    src, dst = ctx.alloc(nb), ctx.alloc(nb)
    src.memset(1); dst.memset(2)
    t = timed(lambda: check(ctx.handle, lib.ah_copy_async(ctx.handle, dst.ptr, src.ptr, nb)))
    res["copy"] = {"bytes": nb, "ms": t, "TB_per_s_read_plus_written": round(2 * nb / (t["median"] * 1e-3) / 1e12, 3)}
    print("copy:", res["copy"]["TB_per_s_read_plus_written"], "TB/s", flush=True)
    src.free(); dst.free()

if "a" in args.only:
    A, B, P, V = ctx.alloc(n * 4 + 64), ctx.alloc(n * 4 + 64), ctx.alloc(n * 8 + 64), ctx.alloc(n * 8 + 64)
    dic, sums, cnts = (ctx.alloc((n + 1) * 8 + 64) for _ in range(3))
    for off in range(0, n, chunk):
        V.upload(rng.integers(-2**40, 2**40, chunk, dtype=np.int64), off * 8)
    res["a"] = {}
    for lg in (10, 16, 20):
        if lg > args.rows_log2:
            continue
        for off in range(0, n, chunk):
            a = rng.integers(0, 1 << (lg // 2), chunk).astype(np.int32) * np.int32(40503) - np.int32(7)
            b = rng.integers(0, 1 << (lg - lg // 2), chunk).astype(np.int32) * np.int32(-2654435)
            A.upload(a, off * 4); B.upload(b, off * 4)
            P.upload(a.view(np.uint32).astype(np.uint64) | (b.view(np.uint32).astype(np.uint64) << np.uint64(32)), off * 8)
        tuple_keys = [(0, 4, 0, None, A, None, 0), (0, 4, 0, None, B, None, 0)]
        r = {"group_ids_tuple_ms": timed(lambda: ctx.group_ids(tuple_keys, n, ids, first)),
             "group_ids_host_packed_ms": timed(lambda: ctx.group_ids([(0, 8, 0, None, P, None, 0)], n, ids, first))}
        ng = ctx.group_ids(tuple_keys, n, ids, first)
        r["groups"] = ng
        r["group_sum_i64_ms"] = timed(lambda: ctx.group_sum("i64", ids, ng, V, None, 0, n, sums, cnts))
        r["hash_sum_i64_host_packed_ms"] = timed(lambda: ctx.hash_sum("i64", P, None, 0, V, None, 0, n, dic, sums, cnts, first))
        ctx.set_option("groupby_partition", 0)
        r["hash_sum_i64_host_packed_idbased_ms"] = timed(lambda: ctx.hash_sum("i64", P, None, 0, V, None, 0, n, dic, sums, cnts, first))
        ctx.set_option("groupby_partition", 1)
        m = lambda k: r[k]["median"]
        r["derived_ms"] = {"new: ids of the tuple + sum over ids": round(m("group_ids_tuple_ms") + m("group_sum_i64_ms"), 4),
                           "before: hash_sum on the host-packed column": m("hash_sum_i64_host_packed_ms"),
                           "the pack pass (tuple ids - host-packed ids)": round(m("group_ids_tuple_ms") - m("group_ids_host_packed_ms"), 4),
                           "no fused route (host-packed ids + sum over ids - hash_sum)": round(m("group_ids_host_packed_ms") + m("group_sum_i64_ms") - m("hash_sum_i64_host_packed_ms"), 4)}
        res["a"][f"2^{lg} groups"] = r
        print(f"a 2^{lg}:", json.dumps(r["derived_ms"]), flush=True)
    for b_ in (A, B, P, V, dic, sums, cnts):
        b_.free()

if "b" in args.only:
    # 2^16 strings of 8 … 24 bytes; one chunk of rows is built on the host and laid out n / chunk times (offsets shifted)
    card = 1 << 16
    pool = rng.integers(97, 123, (card, 24), dtype=np.uint8)
    for j in range(4):
        pool[:, j] = 97 + ((np.arange(card) >> (4 * j)) & 15)                                 # distinct
    plen = rng.integers(8, 25, card)
    pick = rng.integers(0, card, chunk)
    lens = plen[pick]
    rows = pool[pick]
    data = rows[np.arange(24)[None, :] < lens[:, None]]
    coff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cbytes, reps = int(coff[-1]), n // chunk
    assert cbytes * reps < 2**31
    O, D, C = ctx.alloc((n + 1) * 4 + 64), ctx.alloc(cbytes * reps + 64), ctx.alloc(n * 4 + 64)
    for k in range(reps):
        O.upload((coff[:-1] + k * cbytes).astype(np.int32), k * chunk * 4)
        D.upload(data, k * cbytes)
        C.upload((pick & 15).astype(np.int32), k * chunk * 4)
    O.upload(np.array([cbytes * reps], np.int32), n * 4)
    skey = (4, 0, 0, O, D, None, 0)
    r = {"bytes_of_strings": cbytes * reps,
         "hash_binary_encode_ms": timed(lambda: ctx.hash_binary_encode(4, O, D, None, 0, n, True, ids, None, first)),
         "group_ids_string_ms": timed(lambda: ctx.group_ids([skey], n, ids, first)),
         "group_ids_string_int32_ms": timed(lambda: ctx.group_ids([skey, (0, 4, 0, None, C, None, 0)], n, ids, first))}
    r["groups"] = [ctx.group_ids([skey], n, ids, first), ctx.group_ids([skey, (0, 4, 0, None, C, None, 0)], n, ids, first)]
    res["b"] = r
    print("b:", {k: (v["median"] if isinstance(v, dict) else v) for k, v in r.items()}, flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
