"""The LZ4 block compressor and the frame layout behind the IPC writer's device compression, without a GPU.

csrc/ah_lz4_enc.h is compiled for the host into tests/lz4_enc_harness.cc — the 64 lanes of the device's wavefront run one after the
other — with AddressSanitizer and UBSan, and fed hex vectors on stdin; nothing is loaded into Python under a sanitizer.  What comes
out is judged by three readers that share no code with it: the block decoder of tests/lz4_model.py, liblz4 through pyarrow's
codec, and a parser of the sequences (tests/lz4_enc_vectors.py) that checks the encoder-side rules of the block format."""
import os
import shutil
import struct
import subprocess
import tempfile

import pyarrow as pa
import pytest

from tests import lz4_enc_vectors as EV
from tests import lz4_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_harness(directory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    exe = os.path.join(directory, "lz4_enc_harness")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                        os.path.join(ROOT, "tests", "lz4_enc_harness.cc")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and not p.stderr, f"exit {p.returncode}\n{p.stdout[-300:]}\n{p.stderr[-3000:]}"
        out = p.stdout.splitlines()
        assert len(out) == len(lines)
        return out

    return run


def compress_lines(datas, src_mis=0, dst_mis=0):
    return [f"C {src_mis} {dst_mis} {d.hex() or '-'}" for d in datas]


def compressed(answer):
    """→ (stored, size as an LZ4 block, bytes written)"""
    stored, size, payload = answer.split()
    return stored == "1", int(size), (b"" if payload == "-" else bytes.fromhex(payload))


@pytest.fixture(scope="module")
def harness():
    d = tempfile.mkdtemp(prefix="lz4_enc_harness_")
    yield build_harness(d)
    shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="module")
def answers(harness):
    """every vector compressed once: {name: (data, stored, lz4 size, bytes)}"""
    vecs = EV.vectors()
    out = harness(compress_lines([d for _, d in vecs]))
    return {name: (data, *compressed(a)) for (name, data), a in zip(vecs, out)}


NAMES = [name for name, _ in EV.vectors()]


@pytest.mark.parametrize("name", NAMES)
def test_block_inflates_and_keeps_the_format_rules(answers, name):
    data, stored, size, out = answers[name]
    n = len(data)
    assert len(out) <= n, "a block never exceeds its raw size (its slot)"
    if stored:
        assert size >= n and out == data            # reported because it did not shrink, and the slot holds the input
    else:
        assert size == len(out) < n
        assert M.decode_block(out, n) == data
        EV.parse_sequences(out, n)
    frame = M.frame([(out, stored)] if n else [])
    assert pa.Codec("lz4").decompress(frame, decompressed_size=n).to_pybytes() == data


def test_blocks_under_13_bytes_have_no_match(answers):
    for name, (data, stored, size, out) in answers.items():
        if len(data) < 13:
            assert stored and size == len(data) + 1, name   # one token and the literals


def test_compressible_vectors_are_compressed(answers):
    """the vectors that can only come back smaller: a compressor that stores everything passes every other test here"""
    for name in ("zeros_4096", "zeros_65536", "text_4095", "alphabet4_65536", "period_1_full", "period_3_full", "period_64_full", "period_65_full",
                 "period_4097_full", "period_65", "match_into_the_last_12", "match_ends_5_before_the_end", "int64_counter", "string_data",
                 "match_len_273", "literal_run_270", "zeros_64", "zeros_63"):
        data, stored, size, out = answers[name]
        assert not stored and len(out) < len(data), name
    assert len(answers["zeros_65536"][3]) <= 512      # one sequence with ~257 length bytes and at most a step of literals
    for period in (1, 3, 64, 65, 4097):               # the pattern once, a step of literals, one long match
        assert len(answers[f"period_{period}_full"][3]) <= period + 64 + 512
    assert answers["uniform_random"][1] and answers["uniform_random_1000"][1]


def test_end_of_block_matches(answers):
    data, stored, size, out = answers["match_into_the_last_12"]
    seqs = EV.parse_sequences(out, len(data))
    assert seqs[-2][3] + seqs[-2][2] == len(data) - 5 and seqs[-1][0] == 5     # cut 5 bytes before the end
    data, stored, size, out = answers["match_ends_5_before_the_end"]
    seqs = EV.parse_sequences(out, len(data))
    assert seqs[-2][3] + seqs[-2][2] == len(data) - 5 and seqs[-1][0] == 5     # … and one that ends there by itself


@pytest.mark.parametrize("length", [18, 19, 273, 274])
def test_match_length_extension_edges(answers, length):
    data, stored, size, out = answers[f"match_len_{length}"]
    assert not stored and length in [s[2] for s in EV.parse_sequences(out, len(data))]


@pytest.mark.parametrize("run", [14, 15, 270])
def test_literal_length_extension_edges(answers, run):
    data, stored, size, out = answers[f"literal_run_{run}"]
    assert not stored and run in [s[0] for s in EV.parse_sequences(out, len(data))[:-1]]


def test_bytes_do_not_depend_on_where_the_block_and_its_slot_lie(harness, answers):
    names = ["zeros_65", "alphabet4_4095", "text_65535", "period_65", "string_data", "uniform_random_1000", "match_len_274"]
    for src_mis, dst_mis in ((5, 0), (0, 5), (15, 9)):
        out = harness(compress_lines([answers[k][0] for k in names], src_mis, dst_mis))
        for k, a in zip(names, out):
            assert compressed(a) == answers[k][1:], (k, src_mis, dst_mis)


def test_long_literal_runs_cross_the_output_window(harness):
    """more literals than the 4 KiB output window holds, in front of a match: the window is drained in the middle of a sequence"""
    import numpy as np
    noise = np.random.default_rng(5).integers(0, 256, 9000, dtype=np.uint8).tobytes()
    data = noise + bytes(30000) + noise[:5000] + bytes(100)
    (a,) = harness(compress_lines([data], 3, 7))
    stored, size, out = compressed(a)
    assert not stored and M.decode_block(out, len(data)) == data
    assert max(s[0] for s in EV.parse_sequences(out, len(data))) >= 8000


# ---- the frame layout ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("at,sizes", [(0, []), (8, [10]), (64, [65536, 65536, 123]), (16, [1, 2, 3, 4, 5, 6, 7, 8]), (8, [65531])])
def test_frame_layout_against_the_model(harness, at, sizes):
    (a,) = harness([f"L {at} " + " ".join(map(str, sizes))])
    f = a.split()
    prefix_at, header_at, end_mark_at, end, padded_end = int(f[0]), int(f[1]), int(f[3]), int(f[4]), int(f[5])
    head, block_at = bytes.fromhex(f[2]), [int(x) for x in f[6:]]
    # the same buffer put together by the model: prefix, frame of blocks with recognisable bytes, padding
    blocks = [(bytes([i + 1]) * s, i % 2 == 1) for i, s in enumerate(sizes)]
    frame = M.frame(blocks)
    body = bytes(at) + struct.pack("<q", sum(sizes)) + frame
    assert prefix_at == at and header_at == at + 8 and head == frame[:7] and head[4] == 0x60 and head[5] == 0x40
    assert head[6] == (M.xxh32(head[4:6]) >> 8) & 0xFF
    assert len(block_at) == len(sizes) and end == len(body) and padded_end == -(-end // 8) * 8 and end_mark_at == end - 4
    for (data, stored), b in zip(blocks, block_at):
        assert struct.unpack_from("<I", body, b)[0] == len(data) | (0x80000000 if stored else 0) and body[b + 4:b + 4 + len(data)] == data
    flg, bd, parsed, stop = M.parse_frame(body[header_at:])
    assert parsed == blocks and header_at + stop == end


# ---- the layers above ---------------------------------------------------------------------------------------------------------------
def test_exports_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "arrowhip.h")).read()
    source = open(os.path.join(ROOT, "arrow_go_amd", "csrc", "ah_lz4_enc.hip")).read()
    native = open(os.path.join(ROOT, "arrow_go_amd", "_native.py")).read()
    for symbol in ("ah_lz4_compress_blocks", "ah_ipc_pack_body"):
        assert f"int {symbol}(" in header and f"AH_EXPORT int {symbol}(" in source and f'"{symbol}"' in native
    from arrow_go_amd import device as D
    assert callable(D.Context.lz4_compress_blocks) and callable(D.Context.ipc_pack_body)
