"""A host model of the window functions, independent of the library: plain Python and numpy.

The row order comes from Arrow C++ (pc.sort_indices, stable, with the partition id as the first key); everything after that is an
explicit loop over the sorted positions.  Integer sums wrap in numpy's own 64-bit arithmetic; float sums are exact
fractions.Fraction values (the tests compare them with a derived bound, or byte for byte where every prefix sum is an integer
below 2^53); minima and maxima ignore NaNs unless every valid value so far is one, and put -0.0 below +0.0.

  partition_ids(columns)                    dense ids, rows equal when their bytes are (a null is a value of its column)
  sort_order(n, pids, order_columns)        the stable order of (partition id, order keys); the identity without either
  flags(pids, key_lists, order)             per sorted position: bit 0 a partition starts, bit 1 a peer group starts
  ranks(flags, order)                       row_number, rank, dense_rank by ROW (uint64)
  running(op, values, valid, flags, order)  cumulative sum / min / max / count by ROW
  window(batch, partition_by, order_by, functions)   all of it over a record batch: {output name: (values, valid or None)}
"""
import math
import struct
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc


def tie(a, b) -> bool:
    """do two values of an order key tie, as the sort's comparator ties them?"""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) and isinstance(b, float) and (a != a or b != b):
        return a != a and b != b
    return a == b   # -0.0 == +0.0; bytes, str and Decimal by value


def _byte_key(arr):
    """the values of a partition column as hashable stand-ins for their bytes"""
    vals = arr.to_pylist()
    if pa.types.is_floating(arr.type):
        fmt = "<f" if arr.type == pa.float32() else "<d"
        return [None if v is None else struct.pack(fmt, v) for v in vals]
    return vals


def partition_ids(columns, n):
    if not columns:
        return None
    keys = [_byte_key(c) for c in columns]
    seen, ids = {}, []
    for i in range(n):
        k = tuple((col[i] is None, col[i]) for col in keys)
        ids.append(seen.setdefault(k, len(seen)))
    return ids


def sort_order(n, pids, order_columns):
    """order_columns: [(array, 'asc' | 'desc', 'at_end' | 'at_start'), ...]"""
    if pids is None and not order_columns:
        return list(range(n))
    cols, keys = {}, []
    if pids is not None:
        cols["p"] = pa.array(pids, pa.int32())
        keys.append(("p", "ascending", "at_end"))
    for i, (arr, o, npl) in enumerate(order_columns):
        cols["k%d" % i] = arr
        keys.append(("k%d" % i, "ascending" if o == "asc" else "descending", npl))
    return pc.sort_indices(pa.table(cols), sort_keys=keys).to_pylist()


def flags(pids, key_lists, order):
    out = []
    for p, r in enumerate(order):
        if p == 0:
            out.append(3)
            continue
        q = order[p - 1]
        part = pids is not None and pids[q] != pids[r]
        peer = part or not key_lists
        for k in key_lists:
            if peer:
                break
            peer = not tie(k[q], k[r])
        out.append((1 if part else 0) | (2 if peer else 0))
    return out


def ranks(fl, order):
    n = len(order)
    row_number, rank, dense = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    start = peer = d = 0
    for p, r in enumerate(order):
        if fl[p] & 1:
            start, d = p, 0
        if fl[p] & 3:
            peer = p
            d += 1
        row_number[r], rank[r], dense[r] = p - start + 1, peer - start + 1, d
    return row_number, rank, dense


def _less(a, b):
    """a < b with -0.0 < +0.0"""
    if a == b == 0 and isinstance(a, float):
        return math.copysign(1.0, a) < math.copysign(1.0, b)
    return a < b


def running(op, values, valid, fl, order):
    """values: a numpy array by row; valid: numpy bools by row or None.  → by row: op 'count' int64; 'sum' int64 / uint64 (wrapping)
    or a list of Fractions (floats; 0 under a null); 'min' / 'max' the input dtype, 0 under a null."""
    n = len(order)
    dt = values.dtype if values is not None else None
    ok = (lambda r: True) if valid is None else (lambda r: bool(valid[r]))
    if op == "count":
        out, c = np.zeros(n, np.int64), 0
        for p, r in enumerate(order):
            if fl[p] & 1:
                c = 0
            c += ok(r)
            out[r] = c
        return out
    if op == "sum" and dt.kind == "f":
        out, acc = [Fraction(0)] * n, Fraction(0)
        for p, r in enumerate(order):
            if fl[p] & 1:
                acc = Fraction(0)
            if ok(r):
                acc += Fraction(float(values[r]))
                out[r] = acc
        return out
    if op == "sum":
        wide = np.int64 if dt.kind == "i" else np.uint64
        out, acc = np.zeros(n, wide), wide(0)
        with np.errstate(over="ignore"):
            for p, r in enumerate(order):
                if fl[p] & 1:
                    acc = wide(0)
                if ok(r):
                    acc = acc + wide(values[r])
                    out[r] = acc
        return out
    assert op in ("min", "max")
    out = np.zeros(n, dt)
    best, any_valid = None, False   # best: over the values that are not NaN
    pyvals = values.tolist()
    for p, r in enumerate(order):
        if fl[p] & 1:
            best, any_valid = None, False
        if not ok(r):
            continue
        v = pyvals[r]
        any_valid = True
        if v == v and (best is None or (_less(v, best) if op == "min" else _less(best, v))):
            best = v
        out[r] = np.nan if best is None else best
    return out


SUM_TYPE = {"i": pa.int64(), "u": pa.uint64(), "f": pa.float64()}


def window(batch, partition_by=(), order_by=(), functions=()):
    """→ {output name: (values by row, valid by row or None)} in the order of `functions`; order_by: (name, 'asc' | 'desc',
    'at_end' | 'at_start') tuples; functions: 'row_number' | 'rank' | 'dense_rank' and (column, 'cumulative_<op>') pairs"""
    n = batch.num_rows
    col = lambda name: batch.column(batch.schema.names.index(name))
    pids = partition_ids([col(p) for p in partition_by], n)
    order = sort_order(n, pids, [(col(k[0]), k[1], k[2]) for k in order_by])
    fl = flags(pids, [col(k[0]).to_pylist() for k in order_by], order)
    rk = ranks(fl, order)
    out = {}
    for f in functions:
        if isinstance(f, str):
            out[f] = (rk[("row_number", "rank", "dense_rank").index(f)], None)
            continue
        c = col(f[0])
        valid = None if c.null_count == 0 else np.array(c.is_valid().to_pylist(), bool)
        values = c.fill_null(0).to_numpy(zero_copy_only=False)
        op = f[1].replace("cumulative_", "")
        out["%s_%s" % (f[0], f[1])] = (running(op, values, valid, fl, order), None if op == "count" else valid)
    return out
