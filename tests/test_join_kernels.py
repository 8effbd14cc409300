"""The join kernels over caller-supplied dense group ids (csrc/ah_join.hip: ah_join_build, ah_join_count, ah_join_expand,
ah_join_match_bits), DESIGN.md §3.2a, through the C ABI with hand-made ids.

The yardstick is a numpy model: a stable argsort of the ids for the build side, bincount / cumsum for the starts and the offsets,
repeat for the expansion.  Every output is compared BY BYTES; every output buffer starts filled with 0xA5 and is read back past its
end, so a store behind the last entry, or into a buffer the call must not touch, shows."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow_go_amd", "csrc")
SYMBOLS = {"ah_join_build": 8, "ah_join_count": 9, "ah_join_expand": 14, "ah_join_match_bits": 7}
T = 2048          # output slots per workgroup of ah_join_expand (kExpandTile): the tile the cases below cross
SENTINEL = 0xA5
TAIL = 5          # entries read back behind the end of every output


# ---- no GPU needed ------------------------------------------------------------------------------------------------------------------
def test_the_tile_is_the_kernels_tile():
    m = re.search(r"constexpr int kExpandTile = (\d+);", open(os.path.join(CSRC, "ah_join.hip")).read())
    assert m and int(m.group(1)) == T


def test_entry_points_are_declared_exported_and_bound():
    from arrow_go_amd import _native as N
    from arrow_go_amd import device as D
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for sym, nargs in SYMBOLS.items():
        assert sym in N.declared_symbols() and sym in exported, sym
        assert len(getattr(N.lib, sym).argtypes) == nargs, sym
    for name in ("join_build", "join_count", "join_expand", "join_match_bits"):
        assert callable(getattr(D.Context, name))


def test_hash_join_is_registered():
    from arrow_go_amd import compute as ac
    assert ac.has_function("hash_join")
    assert ac.function_num_kernels("hash_join") == 0   # a meta function


def test_expand_is_plain_hip_without_atomics():
    """the hot path has no device-scope atomic, no inline assembly and no wait loop: a tile depends on the inputs alone"""
    src = open(os.path.join(CSRC, "ah_join.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\batomic\w*\s*\(|__hip_atomic|\basm\b|\bwhile\s*\(\s*(true|1)\s*\)", code)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def model(bids, bvalid, pids, pvalid, ng, emit):
    bids, pids = np.asarray(bids, np.int64), np.asarray(pids, np.int64)
    key = np.where(bvalid, bids, ng)
    order = np.argsort(key, kind="stable").astype(np.int64)
    nvalid = int(np.count_nonzero(bvalid))
    counts = np.bincount(bids[bvalid], minlength=ng).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    real = np.where(pvalid, counts[pids] if len(pids) else 0, 0).astype(np.int64) if ng else np.zeros(len(pids), np.int64)
    m = np.maximum(real, 1) if emit else real
    offsets = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
    total = int(offsets[-1])
    prow = np.repeat(np.arange(len(pids), dtype=np.int64), m)
    matched = real[prow] > 0
    k = np.arange(total, dtype=np.int64) - offsets[prow]
    brow = np.zeros(total, np.int64)
    brow[matched] = order[starts[pids[prow[matched]]] + k[matched]]
    return dict(order=order, nvalid=nvalid, starts=starts, offsets=offsets, total=total, prow=prow, brow=brow, matched=matched, hit=real > 0)


def pack(bits):
    return np.packbits(np.asarray(bits, bool), bitorder="little")


class Out:
    """a device buffer of `count` entries of `dtype` followed by TAIL more, all bytes SENTINEL before the call"""

    def __init__(self, ctx, dtype, count, lead_bytes=0):
        self.dtype, self.count, self.lead = np.dtype(dtype), count, lead_bytes
        self.buf = ctx.alloc(lead_bytes + (count + TAIL) * self.dtype.itemsize + 64)
        self.buf.memset(SENTINEL)
        self.ptr = self.buf.at(lead_bytes)

    def read(self, written=None):
        """the first `written` (default: count) entries; everything else must still be the sentinel"""
        written = self.count if written is None else written
        raw = self.buf.download(np.uint8, self.lead + (self.count + TAIL) * self.dtype.itemsize)
        w = self.dtype.itemsize
        assert (raw[:self.lead] == SENTINEL).all(), "wrote in front of the output"
        assert (raw[self.lead + written * w:] == SENTINEL).all(), "wrote behind the last entry"
        return raw[self.lead:self.lead + written * w].view(self.dtype)


def bitmap(ctx, rng, bits, off):
    """`bits` as a device bitmap starting at bit `off`, random bits around them; None for all-valid"""
    if bits is None:
        return None
    around = np.concatenate([rng.random(off) < 0.5, np.asarray(bits, bool), rng.random(13) < 0.5])
    return ctx.to_device(pack(around), 64)


def check_join(ctx, bids, pids, ng, bvalid=None, pvalid=None, voff=0, poff=0, emits=(False, True), lead_bytes=0, seed=0):
    """build, count, expand (with every emit_unmatched of `emits`) and match_bits of one pair of id vectors, against the model"""
    rng = np.random.default_rng(seed)
    bids, pids = np.asarray(bids, np.int32), np.asarray(pids, np.int32)
    nb, npb = len(bids), len(pids)
    bv = np.ones(nb, bool) if bvalid is None else np.asarray(bvalid, bool)
    pv = np.ones(npb, bool) if pvalid is None else np.asarray(pvalid, bool)
    d_bids, d_pids = ctx.to_device(bids, 64), ctx.to_device(pids, 64)
    d_bv, d_pv = bitmap(ctx, rng, bvalid, voff), bitmap(ctx, rng, pvalid, poff)
    starts, rows = Out(ctx, np.int64, ng + 1), Out(ctx, np.int64, nb)
    ctx.join_build(d_bids, d_bv, voff, nb, ng, starts.ptr, rows.ptr)
    want = model(bids, bv, pids, pv, ng, False)
    got_starts = starts.read()
    assert got_starts.tobytes() == want["starts"].tobytes()
    got_rows = rows.read(nb if nb else 0)
    assert got_rows[:want["nvalid"]].tobytes() == want["order"][:want["nvalid"]].tobytes()
    assert int(got_starts[ng]) == want["nvalid"]
    for emit in emits:
        want = model(bids, bv, pids, pv, ng, emit)
        total = want["total"]
        offsets = Out(ctx, np.int64, npb + 1)
        assert ctx.join_count(d_pids, d_pv, poff, npb, starts.ptr, emit, offsets.ptr) == total
        assert offsets.read().tobytes() == want["offsets"].tobytes()
        prow, brow = Out(ctx, np.int64, total, lead_bytes), Out(ctx, np.int64, total, lead_bytes)
        valid = Out(ctx, np.uint8, (total + 7) // 8)
        nulls = ctx.join_expand(d_pids, d_pv, poff, npb, starts.ptr, rows.ptr, offsets.ptr, total, emit, prow.ptr, brow.ptr, valid.ptr)
        assert prow.read().tobytes() == want["prow"].tobytes()
        assert brow.read().tobytes() == want["brow"].tobytes()
        if emit:
            assert valid.read().tobytes() == pack(want["matched"]).tobytes()   # packbits pads the last byte with zeros
            assert nulls == int(np.count_nonzero(~want["matched"]))
        else:
            valid.read(0)                                                      # not touched
            assert nulls == 0
        for o in (offsets, prow, brow, valid):
            o.buf.free()
    bits = Out(ctx, np.uint8, (npb + 7) // 8)
    ctx.join_match_bits(d_pids, d_pv, poff, npb, starts.ptr, bits.ptr)
    assert bits.read().tobytes() == pack(want["hit"]).tobytes()
    for b in (d_bids, d_pids, d_bv, d_pv, starts.buf, rows.buf, bits.buf):
        if b is not None:
            b.free()
    return want


@pytest.fixture(scope="module")
def ctx():
    import arrow_go_amd as ah
    with ah.Context(0) as c:
        yield c


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("total", [T - 1, T, T + 1, 3 * T + 5])
def test_totals_around_the_tile(ctx, total):
    # one match per probe row: as many probe rows as output slots
    rng = np.random.default_rng(total)
    assert check_join(ctx, rng.permutation(total), rng.permutation(total), total, emits=(False,))["total"] == total
    # runs of three, the last shorter: runs straddle the tile boundaries
    bids = [0, 0, 0] + [1] * (total % 3)
    pids = [0] * (total // 3) + [1] * (1 if total % 3 else 0)
    assert check_join(ctx, bids, pids, 2)["total"] == total
    # the same at an output address that is 8 but not 16 bytes aligned
    assert check_join(ctx, bids, pids, 2, lead_bytes=8, emits=(True,))["total"] == total


@pytest.mark.gpu
def test_one_probe_row_whose_run_spans_more_than_three_tiles(ctx):
    assert check_join(ctx, [0] * (3 * T + 5), [0], 1)["total"] == 3 * T + 5
    # ... with neighbours on both sides, and rows in front of the run that match nothing
    assert check_join(ctx, [1] + [0] * (3 * T + 5) + [1], [2, 1, 2, 0, 1], 3, emits=(False,))["total"] == 3 * T + 9


@pytest.mark.gpu
def test_a_long_stretch_of_probe_rows_without_a_match_is_skipped(ctx):
    empty = T + 500
    want = check_join(ctx, [0, 0], [0] + [1] * empty + [0], 2, emits=(False,))
    assert want["total"] == 4
    # the same stretch under cleared validity bits, with ids that WOULD match; and several stretches inside a larger call
    pvalid = np.array([True] + [False] * empty + [True])
    assert check_join(ctx, [0, 0], [0] * (empty + 2), 1, pvalid=pvalid, poff=3, emits=(False,))["total"] == 4
    pids = np.concatenate([[0] * 700, [1] * (2 * T + 7), [0] * 900, [1] * (T + 1), [0] * 600])
    assert check_join(ctx, [0, 0, 0], pids, 2, emits=(False,))["total"] == 3 * 2200


@pytest.mark.gpu
@pytest.mark.parametrize("emit", [False, True])
def test_run_lengths_0_1_2_1000_in_one_call(ctx, emit):
    rng = np.random.default_rng(7)
    bids = rng.permutation(np.array([1] + [2] * 2 + [3] * 1000))
    pids = rng.integers(0, 4, 300)
    want = check_join(ctx, bids, pids, 4, emits=(emit,))
    assert want["total"] > 50 * 1000 and (np.bincount(pids, minlength=4) > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1, 3, 7])
def test_validity_bitmaps_at_bit_offsets(ctx, off):
    """a row under a cleared bit whose id would match must not match — on either side"""
    rng = np.random.default_rng(10 + off)
    nb, npb, ng = 3001, 2999, 97
    bids, pids = rng.integers(0, ng, nb), rng.integers(0, ng, npb)
    bvalid, pvalid = rng.random(nb) < 0.8, rng.random(npb) < 0.8
    want = check_join(ctx, bids, pids, ng, bvalid=bvalid, pvalid=pvalid, voff=off, poff=(off * 5) % 8, seed=off)
    would = np.bincount(bids, minlength=ng)[pids] > 0
    assert np.count_nonzero(would & ~want["hit"]) > 100   # the case bites: rows that only the validity bits keep from matching
    check_join(ctx, bids, pids, ng, bvalid=bvalid, voff=off, emits=(True,), seed=off)    # one side only
    check_join(ctx, bids, pids, ng, pvalid=pvalid, poff=off, emits=(False,), seed=off)


@pytest.mark.gpu
def test_the_build_validity_of_a_left_outer_expansion(ctx):
    """tail bits of the last byte 0, null count = the model's, for totals that end inside a byte and on a byte"""
    rng = np.random.default_rng(3)
    for npb in (1, 7, 8, 9, 63, 64, 65, 1000, T + 3):
        pids = rng.integers(0, 5, npb)
        want = check_join(ctx, [0, 2, 4], pids, 5, emits=(True,))     # one match or none: total = npb
        assert want["total"] == npb
    want = check_join(ctx, [0, 0, 2], rng.integers(0, 5, 500), 5, pvalid=rng.random(500) < 0.7, poff=5, emits=(True,))
    assert 0 < np.count_nonzero(~want["matched"]) < want["total"]


@pytest.mark.gpu
def test_degenerate_sizes(ctx):
    assert check_join(ctx, [], [0, 1, 2, 1], 3)["total"] == 4                       # no build rows: nothing, then four unmatched rows
    assert check_join(ctx, [0, 1, 1], [], 2)["total"] == 0                          # no probe rows
    assert check_join(ctx, [], [], 0)["total"] == 0                                 # nothing at all
    assert check_join(ctx, [0, 0, 1], [2, 3, 2], 4, emits=(False,))["total"] == 0   # rows on both sides, no key in common
    assert check_join(ctx, [0] * 300, [0] * 300, 1)["total"] == 90000               # every row in one group
    assert check_join(ctx, [0], [0], 1)["total"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [1, 7, 5000])
def test_build_keeps_the_rows_of_a_group_in_row_order(ctx, ng):
    rng = np.random.default_rng(ng)
    n = 5000
    bids = rng.integers(0, ng, n).astype(np.int32) if ng < n else rng.permutation(n).astype(np.int32)
    bvalid = rng.random(n) < 0.9
    d_ids, d_valid = ctx.to_device(bids, 64), bitmap(ctx, rng, bvalid, 5)
    starts, rows = Out(ctx, np.int64, ng + 1), Out(ctx, np.int64, n)
    ctx.join_build(d_ids, d_valid, 5, n, ng, starts.ptr, rows.ptr)
    s, r = starts.read(), rows.read()
    nvalid = int(np.count_nonzero(bvalid))
    assert s[0] == 0 and s[ng] == nvalid and (np.diff(s) >= 0).all()
    for g in range(ng):
        mine = r[s[g]:s[g + 1]]
        assert (bids[mine] == g).all() and bvalid[mine].all() and (np.diff(mine) > 0).all(), g
    assert sorted(r[:nvalid]) == sorted(np.flatnonzero(bvalid))
    want = model(bids, bvalid, [], [], ng, False)
    assert s.tobytes() == want["starts"].tobytes() and r[:nvalid].tobytes() == want["order"][:nvalid].tobytes()
    for b in (d_ids, d_valid, starts.buf, rows.buf):
        b.free()
