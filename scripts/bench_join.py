"""hash_join on three shapes, one Int64 key and one Int64 payload column per side, inner join, ms per phase.

  fk      2^R left rows with random keys into 2^R right rows with unique keys (foreign-key shape: about 2^R output rows)
  fanout  2^R left rows over 2^10 distinct keys, 2^10 x 16 right rows, every key 16 times (2^(R+4) output rows: write-bound)
  skew    2^(R-2) left rows, half of them ONE key that has 64 right rows, the other half random keys into 2^(R-2) - 64 unique right
          rows (about 2^(R+3) output rows, almost all of them from one key): per output row this is to be read beside `fanout`

Phases, through the C ABI as HashJoinImpl (host/kernels.cc) calls it — the key columns are already laid end to end:
  ids     ah_group_ids over the n_left + n_right keys          build   ah_join_build on the right side's ids
  count   ah_join_count on the left side's ids                 expand  ah_join_expand
  takes   three ah_take_primitive calls: left key and left payload by the probe rows, right payload by the build rows
and `call`, the host clock around Session.hash_join(..., keep_on_device=True) on device-resident batches, which adds the
Concatenate of the keys, the allocations and the datum plumbing.

expand is set against its own traffic: 4 B read per probe row + 8 B gathered from `rows` per output slot + 16 B written per output
slot, over the kernel's time, as a fraction of the copy rate (ah_copy_async of 512 MiB, bytes read + written per second) measured in
the same run.  pyarrow's Table.join on the same tables on the same machine is listed as context, with the cores it could use.

Every figure is the median of ROUNDS windows between two device events (phases that synchronise are timed the same way: the
events are on the stream), after WARM warm-ups; "spread" is (max - min) / median.
      python scripts/bench_join.py [--rows-log2 24] [--out profiles/join_bench.json] [--no-pyarrow]
"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arrow_go_amd as ah
from arrow_go_amd._native import lib, check

WARM, ROUNDS = 1, 5
ap = argparse.ArgumentParser()
ap.add_argument("--rows-log2", type=int, default=24)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "join_bench.json"))
ap.add_argument("--no-pyarrow", action="store_true")
args = ap.parse_args()
if ah.device_count() < 1:
    raise SystemExit("bench_join: no GPU visible")
ctx = ah.Context(0)
R = args.rows_log2
rng = np.random.default_rng(1)


def timed(fn, rounds=ROUNDS, warm=WARM):
    for _ in range(warm): fn()
    xs = []
    for _ in range(rounds):
        ctx.sync(); ctx.event_record(1)
        fn()
        ctx.event_record(2); ctx.sync()
        xs.append(round(ctx.event_elapsed_ms(1, 2), 4))
    med = float(np.median(xs))
    return {"median": round(med, 4), "min": min(xs), "max": max(xs), "spread": round((max(xs) - min(xs)) / med, 4), "rounds": xs}


def shapes():
    n = 1 << R
    yield "fk", rng.integers(0, n, n).astype(np.int64), rng.permutation(n).astype(np.int64)
    yield "fanout", rng.integers(0, 1 << 10, n).astype(np.int64), rng.permutation(np.repeat(np.arange(1 << 10, dtype=np.int64), 16))
    m = n >> 2
    hot = np.int64(-1)
    left = np.where(rng.random(m) < 0.5, hot, rng.integers(0, m - 64, m)).astype(np.int64)
    yield "skew", left, rng.permutation(np.concatenate([np.full(64, hot), np.arange(m - 64, dtype=np.int64)]))


res = {"what": f"scripts/bench_join.py: inner hash_join, Int64 key + Int64 payload per side, 2^{R} rows (skew: 2^{R - 2}), ms", "warmups": WARM, "rounds": ROUNDS,
       "cpu_count": os.cpu_count(), "cpus_usable": len(os.sched_getaffinity(0)), "shapes": {}}
nb = 512 << 20
src, dst = ctx.alloc(nb), ctx.alloc(nb)
src.memset(1); dst.memset(2)
t = timed(lambda: check(ctx.handle, lib.ah_copy_async(ctx.handle, dst.ptr, src.ptr, nb)), rounds=7, warm=2)
copy_rate = 2 * nb / (t["median"] * 1e-3)
res["copy"] = {"bytes": nb, "ms": t, "TB_per_s_read_plus_written": round(copy_rate / 1e12, 3)}
print("copy:", res["copy"]["TB_per_s_read_plus_written"], "TB/s", flush=True)
src.free(); dst.free()

for name, lkeys, rkeys in shapes():
    nl, nr = len(lkeys), len(rkeys)
    lpay, rpay = np.arange(nl, dtype=np.int64), np.arange(nr, dtype=np.int64) * 3
    keys = ctx.to_device(np.concatenate([lkeys, rkeys]), 64)
    d_lpay, d_rpay = ctx.to_device(lpay, 64), ctx.to_device(rpay, 64)
    ids, first = ctx.alloc((nl + nr) * 4 + 64), ctx.alloc((nl + nr + 1) * 8 + 64)
    out = {"n_left": nl, "n_right": nr}
    ng = ctx.group_ids([(0, 8, 0, None, keys, None, 0)], nl + nr, ids, first)
    out["ids"] = timed(lambda: ctx.group_ids([(0, 8, 0, None, keys, None, 0)], nl + nr, ids, first))
    starts, rows = ctx.alloc((ng + 1) * 8 + 64), ctx.alloc(nr * 8 + 64)
    lids, rids = ids.at(0), ids.at(nl * 4)
    out["build"] = timed(lambda: ctx.join_build(rids, None, 0, nr, ng, starts, rows))
    offsets = ctx.alloc((nl + 1) * 8 + 64)
    total = ctx.join_count(lids, None, 0, nl, starts, False, offsets)
    out["count"] = timed(lambda: ctx.join_count(lids, None, 0, nl, starts, False, offsets))
    prow, brow = ctx.alloc(total * 8 + 64), ctx.alloc(total * 8 + 64)
    out["expand"] = timed(lambda: ctx.join_expand(lids, None, 0, nl, starts, rows, offsets, total, False, prow, brow, None))
    traffic = 4 * nl + (8 + 16) * total
    rate = traffic / (out["expand"]["median"] * 1e-3)
    out.update(groups=ng, output_rows=total, expand_bytes=traffic, expand_TB_per_s=round(rate / 1e12, 3),
               expand_fraction_of_copy=round(rate / copy_rate, 3))
    # the result against numpy, once, before anything is timed on top of it (keys shifted by one: the hot key is -1)
    m = np.bincount(rkeys + 1, minlength=int(max(lkeys.max(), rkeys.max())) + 2)[lkeys + 1]
    got_l, got_r = prow.download(np.int64, total), brow.download(np.int64, total)
    assert total == int(m.sum()) and (got_l == np.repeat(np.arange(nl, dtype=np.int64), m)).all(), "expand: not the model's probe rows"
    assert (lkeys[got_l] == rkeys[got_r]).all(), "expand: a pair with unequal keys"
    assert (np.diff(got_r)[np.diff(got_l) == 0] > 0).all(), "expand: the matches of one left row are not in ascending row order"
    del got_l, got_r, m
    tk = [ctx.alloc(total * 8 + 64) for _ in range(3)]

    def takes():
        ctx.take_primitive(8, keys, None, 0, nl, 8, True, prow, None, 0, total, False, tk[0], None)
        ctx.take_primitive(8, d_lpay, None, 0, nl, 8, True, prow, None, 0, total, False, tk[1], None)
        ctx.take_primitive(8, d_rpay, None, 0, nr, 8, True, brow, None, 0, total, False, tk[2], None)
    out["takes"] = timed(takes)
    phases = ("ids", "build", "count", "expand", "takes")
    out["phases_ms"] = round(sum(out[p]["median"] for p in phases), 4)
    out["ns_per_output_row"] = {p: round(out[p]["median"] * 1e6 / total, 4) for p in phases}
    for b in [keys, d_lpay, d_rpay, ids, first, starts, rows, offsets, prow, brow] + tk:
        b.free()
    # the whole call, and pyarrow's on the same tables
    import pyarrow as pa
    from arrow_go_amd import compute as ac
    lt = pa.record_batch({"k": pa.array(lkeys), "lv": pa.array(lpay)})
    rt = pa.record_batch({"k": pa.array(rkeys), "rv": pa.array(rpay)})
    sess = ac.Session(0)

    def upload(batch):   # device-resident batches: an identity filter keeps the columns in HBM
        return sess.call_function("filter", [batch, pa.array(np.ones(batch.num_rows, bool))], keep_on_device=True)
    dl, dr = upload(lt), upload(rt)
    walls = []
    for i in range(WARM + ROUNDS):
        t0 = time.perf_counter()
        r = sess.hash_join(dl, dr, "k", keep_on_device=True)
        last = sess.call_function("take", [r, pa.array([total - 1], pa.int64())])   # one row brought home: everything enqueued before it has run
        assert last.num_rows == 1 and last["k"][0].as_py() == int(lkeys[last["lv"][0].as_py()])
        r.release()
        walls.append(round((time.perf_counter() - t0) * 1e3, 3))
    out["call_wall_ms"] = {"median": float(np.median(walls[WARM:])), "rounds": walls[WARM:], "note": "host clock around the call and the download of its last row"}
    dl.release(); dr.release(); sess.close()
    if not args.no_pyarrow:
        pa.set_cpu_count(min(16, len(os.sched_getaffinity(0))))   # the cores this command may use
        tl, tr = pa.Table.from_batches([lt]), pa.Table.from_batches([rt])
        pw = []
        for i in range(3):
            t0 = time.perf_counter()
            j = tl.join(tr, keys="k", join_type="inner")
            pw.append(round((time.perf_counter() - t0) * 1e3, 1))
            assert j.num_rows == total
            del j
        out["pyarrow_join_wall_ms"] = {"median": float(np.median(pw)), "rounds": pw, "version": pa.__version__, "threads": pa.cpu_count()}
    res["shapes"][name] = out
    print(name, json.dumps({k: (v["median"] if isinstance(v, dict) and "median" in v else v) for k, v in out.items()}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)

a, b = res["shapes"]["fanout"], res["shapes"]["skew"]
res["skew_vs_fanout"] = {"expand_ns_per_output_row": [a["ns_per_output_row"]["expand"], b["ns_per_output_row"]["expand"]],
                         "fanout_expand_spread": a["expand"]["spread"],
                         "ratio": round(b["ns_per_output_row"]["expand"] / a["ns_per_output_row"]["expand"], 3)}
json.dump(res, open(args.out, "w"), indent=1)
print(json.dumps(res["skew_vs_fanout"]))
