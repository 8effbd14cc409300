"""The limb arithmetic of the decimal casts (csrc/ah_decimal.h) on the CPU: the header compiled for the host against Python integers,
≥ 10^5 random and edge rows per routine and width — multiplication by 10^k with its carry out of the top limb, truncated division by
10^k with the two remainder tests (≠ 0, and 2·r ≥ 10^k from r = x − q·10^k), the precision test, negation and increment, and the
comparisons' scale_up.  Edge rows: ±(10^p − 1), ±10^p, the neighbours of 2^127 / 2^255 and of the limb boundaries, remainders of exactly
half, every k = 0 … 38 (two limbs) / 0 … 76 (four limbs)."""
import ctypes as C
import os
import random
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 100_000


@pytest.fixture(scope="module")
def host():
    d = tempfile.mkdtemp(prefix="dech_")
    so = os.path.join(d, "libdech.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-shared", "-fPIC", os.path.join(ROOT, "tests", "decimal_harness.cc"), "-o", so])
    lib = C.CDLL(so)
    vp, lg, it = C.c_void_p, C.c_long, C.c_int
    lib.dh_mul_pow10.argtypes = [it, vp, lg, vp, vp, vp]
    lib.dh_div_pow10.argtypes = [it, vp, lg, vp, vp, vp, vp]
    lib.dh_unary.argtypes = [it, it, vp, lg, vp, vp]
    lib.dh_fits.argtypes = [it, vp, vp, lg, vp]
    lib.dh_scale_up.argtypes = [vp, lg, vp, vp]
    for f in (lib.dh_mul_pow10, lib.dh_div_pow10, lib.dh_unary, lib.dh_fits, lib.dh_scale_up):
        f.restype = None
    return lib


def to_limbs(values, limbs):
    """unsigned Python integers (< 2^(64·limbs)) → a (rows, limbs) uint64 array, little-endian limbs"""
    raw = b"".join(v.to_bytes(8 * limbs, "little") for v in values)
    return np.frombuffer(raw, dtype=np.uint64).reshape(len(values), limbs).copy()


def from_limbs(arr):
    limbs = arr.shape[1]
    raw = arr.tobytes()
    return [int.from_bytes(raw[i * 8 * limbs:(i + 1) * 8 * limbs], "little") for i in range(arr.shape[0])]


def magnitudes(limbs, rng):
    """unsigned values of the width: edges first, then random ones of every bit length"""
    bits = 64 * limbs
    top = 1 << bits
    edges = {0, 1, 2, top - 1, top - 2, top >> 1, (top >> 1) - 1, (top >> 1) + 1}
    for p in range(0, 39 if limbs == 2 else 77):
        edges |= {10 ** p - 1, 10 ** p, 10 ** p + 1, 5 * 10 ** p, 5 * 10 ** p - 1, 5 * 10 ** p + 1}
    for b in range(63, bits, 64):
        edges |= {(1 << b) - 1, 1 << b, (1 << b) + 1, (1 << (b + 1)) - 1, (1 << (b + 1)) % top}
    edges = sorted(e for e in edges if 0 <= e < top)
    out = list(edges)
    while len(out) < ROWS:
        out.append(rng.getrandbits(rng.randint(1, bits)))
    return out, len(edges)


@pytest.mark.parametrize("limbs", [2, 4])
def test_mul_pow10_matches_python_integers(host, limbs):
    rng = random.Random(10 + limbs)
    vals, nedge = magnitudes(limbs, rng)
    kmax = 38 if limbs == 2 else 76
    # edge rows × every k, then the random rows with random k
    rows = [(v, k) for v in vals[:nedge] for k in range(kmax + 1)] + [(v, rng.randint(0, kmax)) for v in vals]
    assert len(rows) >= ROWS
    a = to_limbs([v for v, _ in rows], limbs)
    k = np.array([kk for _, kk in rows], dtype=np.int32)
    out = np.zeros_like(a)
    carry = np.zeros(len(rows), np.uint8)
    host.dh_mul_pow10(limbs, a.ctypes.data, len(rows), k.ctypes.data, out.ctypes.data, carry.ctypes.data)
    got = from_limbs(out)
    top = 1 << (64 * limbs)
    for i, (v, kk) in enumerate(rows):
        exact = v * 10 ** kk
        assert got[i] == exact % top, (v, kk)
        if exact < top:
            assert carry[i] == 0, (v, kk)          # a product that fits never reports a carry
        # a carry out of ANY step is reported; a product that leaves the width always carries in some step
        assert carry[i] == (1 if exact >= top else 0), (v, kk)


@pytest.mark.parametrize("limbs", [2, 4])
def test_div_pow10_matches_python_integers(host, limbs):
    rng = random.Random(20 + limbs)
    vals, nedge = magnitudes(limbs, rng)
    kmax = 38 if limbs == 2 else 76
    top = 1 << (64 * limbs)
    rows = [(v, k) for v in vals[:nedge] for k in range(kmax + 1)] + [(v, rng.randint(0, kmax)) for v in vals]
    # remainders of exactly half, one below and one above it, under random quotients
    for kk in range(1, kmax + 1):
        for _ in range(20):
            q = rng.getrandbits(rng.randint(1, 64 * limbs)) // 10 ** kk
            for r in (10 ** kk // 2 - 1, 10 ** kk // 2, 10 ** kk // 2 + 1, 0, 10 ** kk - 1):
                if q * 10 ** kk + r < top and r >= 0:
                    rows.append((q * 10 ** kk + r, kk))
    assert len(rows) >= ROWS
    a = to_limbs([v for v, _ in rows], limbs)
    k = np.array([kk for _, kk in rows], dtype=np.int32)
    out = np.zeros_like(a)
    nonzero, half = np.zeros(len(rows), np.uint8), np.zeros(len(rows), np.uint8)
    host.dh_div_pow10(limbs, a.ctypes.data, len(rows), k.ctypes.data, out.ctypes.data, nonzero.ctypes.data, half.ctypes.data)
    got = from_limbs(out)
    for i, (v, kk) in enumerate(rows):
        q, r = divmod(v, 10 ** kk)
        assert got[i] == q, (v, kk)
        assert nonzero[i] == (r != 0), (v, kk)
        assert half[i] == (kk > 0 and 2 * r >= 10 ** kk), (v, kk)


@pytest.mark.parametrize("limbs", [2, 4])
def test_negate_increment_sign_and_precision_test(host, limbs):
    rng = random.Random(30 + limbs)
    vals, _ = magnitudes(limbs, rng)
    top = 1 << (64 * limbs)
    a = to_limbs(vals, limbs)
    for op, fn in ((0, lambda v: (-v) % top), (1, lambda v: (v + 1) % top)):
        out = np.zeros_like(a)
        flag = np.zeros(len(vals), np.uint8)
        host.dh_unary(limbs, op, a.ctypes.data, len(vals), out.ctypes.data, flag.ctypes.data)
        got = from_limbs(out)
        for i, v in enumerate(vals):
            assert got[i] == fn(v), (op, v)
            assert flag[i] == (v >= top >> 1), v
    # |v| < 10^p for every p of the width: the edge rows sit on both sides of every bound
    pmax = 38 if limbs == 2 else 76
    bounds = [10 ** rng.randint(1, pmax) for _ in vals]
    for i in range(0, 6 * (pmax + 1)):       # the first rows are the sorted edges: pair each with its own neighbourhood's bound as well
        bounds[i] = 10 ** min(pmax, max(1, len(str(vals[i])) - (i % 2)))
    b = to_limbs(bounds, limbs)
    out = np.zeros(len(vals), np.uint8)
    host.dh_fits(limbs, a.ctypes.data, b.ctypes.data, len(vals), out.ctypes.data)
    for i, v in enumerate(vals):
        assert out[i] == (v < bounds[i]), (v, bounds[i])
    # … and each bound against itself and its two neighbours
    trip = [(10 ** p + d, 10 ** p) for p in range(1, pmax + 1) for d in (-1, 0, 1)]
    a3, b3 = to_limbs([t[0] for t in trip], limbs), to_limbs([t[1] for t in trip], limbs)
    out = np.zeros(len(trip), np.uint8)
    host.dh_fits(limbs, a3.ctypes.data, b3.ctypes.data, len(trip), out.ctypes.data)
    assert out.tolist() == [1, 0, 0] * pmax


def test_scale_up_of_the_comparisons_is_unchanged(host):
    rng = random.Random(7)
    vals, nedge = magnitudes(4, rng)
    rows = [(v, k) for v in vals[:nedge:7] for k in range(77)] + [(v, rng.randint(0, 76)) for v in vals]
    a = to_limbs([v for v, _ in rows], 4)
    k = np.array([kk for _, kk in rows], dtype=np.int32)
    out = np.zeros_like(a)
    host.dh_scale_up(a.ctypes.data, len(rows), k.ctypes.data, out.ctypes.data)
    got = from_limbs(out)
    for i, (v, kk) in enumerate(rows):
        assert got[i] == (v * 10 ** kk) % (1 << 256), (v, kk)
