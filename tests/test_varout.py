"""The four producers of a var-length output share one tail (csrc/ah_varout.h): the temp arena's lens / incl, the overflow word, the
pinned words the total comes home in.  Here they run back to back in ONE context, twice, in interleaved order and at changing row
counts — a binary Take, a binary if_else, an int64 → string cast and a utf8_trim — so that what one call leaves behind (a stale
overflow or count word, pinned words of another layout, arena bytes of a longer column) meets the next.  Bytes against the host
models the producers' own suites use; every returned total against out_offsets[n]."""
import numpy as np
import pytest

from tests import conditional_model as CM
from tests import oracle_lib as OL
from tests import string_transform_model as M
from tests.backends import OracleBackend
from tests.test_conditional_kernels import Cond, Side, guarded, row_lengths
from tests.test_string_transform_kernels import Column, run as run_transform, text

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 4097)   # one lane, around a wave, more than one workgroup of the lengths and offsets kernels
NVALUES, OFF = 300, 3
INT64 = 9   # arrow.Type id


def offsets_and_total(buf, dtype, n, total, what):
    buf.check(what)
    got = buf.download(dtype, n + 1)
    assert total == int(got[n]), (what, "total", total, "out_offsets[n]", int(got[n]))
    return got


def take_case(ctx, n, ow, rng):
    odt = np.int32 if ow == 4 else np.int64
    lens = rng.geometric(1.0 / 8, NVALUES) - 1
    offsets = np.zeros(NVALUES + 1, odt)
    offsets[1:] = np.cumsum(lens)
    data = rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    vvalid = OL.pack_bits(list(rng.random(NVALUES) >= 0.15))
    idx = rng.integers(0, NVALUES, n).astype(np.int32)
    ivalid = OL.pack_bits(list(rng.random(n) >= 0.1)) if n % 2 else None
    status, want_offsets, want_data, want_valid, want_nulls, _ = OracleBackend().take_binary(offsets, data, vvalid, 0, NVALUES, idx, ivalid, 0, True)
    assert status == 0
    d_off, d_data, d_vv, d_idx = ctx.to_device(offsets, pad=8), ctx.to_device(data, pad=16), ctx.to_device(vvalid, pad=8), ctx.to_device(idx, pad=8)
    d_iv = None if ivalid is None else ctx.to_device(ivalid, pad=8)

    def run():
        what = str(("take_binary", n, ow))
        oo, ov = guarded(ctx, (n + 1) * ow, "take offsets"), guarded(ctx, (n + 7) // 8, "take validity")
        nulls, total = ctx.take_binary_offsets(ow, d_off, d_vv, 0, NVALUES, 4, True, d_idx, d_iv, 0, n, oo, ov)
        assert offsets_and_total(oo, odt, n, total, what).tobytes() == want_offsets.tobytes(), what
        ov.check(what)
        assert ov.download(np.uint8, (n + 7) // 8).tobytes() == want_valid.tobytes() and nulls == want_nulls, what
        od = guarded(ctx, total, "take data")
        ctx.take_binary_data(ow, d_off, d_data, 0, 4, d_idx, n, oo, od)
        ctx.sync()
        od.check(what)
        assert od.download(np.uint8, total).tobytes() == want_data.tobytes(), what
    return run


def if_else_case(ctx, n, ow, rng):
    cond = Cond(ctx, "random_nulls", n, 5, rng)
    left = Side(ctx, "binary", n, 1, True, False, rng, ow=4, lengths=row_lengths(n, rng))
    right = Side(ctx, "binary", n, 9, False, False, rng, ow=8, lengths=row_lengths(n, rng))
    want_offsets, want_valid, want_total = CM.if_else_binary_offsets(*cond.model(), left.model, right.model, n, ow)
    want_data = CM.if_else_binary_data(*cond.model(), left.model, right.model, n, want_offsets)

    def run():
        what = str(("if_else_binary", n, ow))
        oo, ov = guarded(ctx, (n + 1) * ow, "if_else offsets"), guarded(ctx, (n + 7) // 8, "if_else validity")
        total = ctx.if_else_binary_offsets(*cond.dev(), left.dev, right.dev, n, ow, oo, ov)
        assert offsets_and_total(oo, want_offsets.dtype, n, total, what).tobytes() == want_offsets.tobytes() and total == want_total, what
        ov.check(what)
        assert ov.download(np.uint8, (n + 7) // 8).tobytes() == np.asarray(want_valid).tobytes(), what
        od = guarded(ctx, total, "if_else data")
        ctx.if_else_binary_data(*cond.dev(), left.dev, right.dev, n, ow, oo, od)
        ctx.sync()
        od.check(what)
        assert od.download(np.uint8, total).tobytes() == np.asarray(want_data).tobytes(), what
    return run


def cast_case(ctx, n, ow, rng):
    odt = np.int32 if ow == 4 else np.int64
    vals = rng.integers(-10 ** 18, 10 ** 18, n).astype(np.int64) >> rng.integers(0, 60, n)   # 1 … 19 digits, a sign or none
    ok = (rng.random(n + OFF) >= 0.1).astype(np.uint8)
    texts = [str(v).encode() if ok[OFF + i] else b"" for i, v in enumerate(vals.tolist())]
    want_offsets = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(odt)
    d_valid = ctx.to_device(np.packbits(ok, bitorder="little"), pad=8)
    d_vals = ctx.to_device(np.concatenate([np.zeros(OFF, np.int64), vals]))

    def run():
        what = str(("format int64", n, ow))
        oo = guarded(ctx, (n + 1) * ow, "format offsets")
        total = ctx.format_int_offsets(INT64, d_vals.ptr + OFF * 8, d_valid, OFF, n, ow, oo)
        assert offsets_and_total(oo, odt, n, total, what).tobytes() == want_offsets.tobytes(), what
        od = guarded(ctx, total, "format data")
        ctx.format_int_data(INT64, d_vals.ptr + OFF * 8, d_valid, OFF, n, ow, oo, od)
        ctx.sync()
        od.check(what)
        assert od.download(np.uint8, total).tobytes() == b"".join(texts), what
    return run


def trim_case(ctx, n, ow, rng):
    rows = [None if rng.random() < 0.1 else text(rng, int(k)) for k in rng.integers(0, 12, n)]
    rows[int(rng.integers(0, n))] = b" x" * 40 + text(rng, 30) + "é ".encode() * 40   # trimmed by the wave on both sides
    col = Column(ctx, rows, ow=ow, off=2, voff=5, rng=rng)
    # (run_transform compares the offsets and the data with the model and the total with the model's last offset)
    return lambda: run_transform(ctx, col, M.TRIM_CODEPOINTS, what="utf8_trim among the var-length producers", sides=M.BOTH, chars="x é".encode())


PRODUCERS = (take_case, if_else_case, cast_case, trim_case)


@pytest.mark.parametrize("ow", [4, 8])
def test_the_four_producers_back_to_back_in_one_context(ctx, ow):
    rng = np.random.default_rng(40 + ow)
    cases = {(p, n): p(ctx, n, ow, rng) for p in PRODUCERS for n in SIZES}   # inputs and references once; every case runs twice
    for order in (PRODUCERS, PRODUCERS[::-1]):
        for i in range(len(SIZES)):
            for k, p in enumerate(order):
                cases[p, SIZES[(i + 2 * k) % len(SIZES)]]()   # neighbours differ in n: the arena's bytes are another column's
