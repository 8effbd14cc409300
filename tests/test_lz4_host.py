"""The LZ4 block decoder and frame planner behind the IPC reader's device inflate, without a GPU.

csrc/ah_lz4.h is compiled for the host into tests/lz4_harness.cc — the 64 lanes of the device's wavefront run one after the other —
with AddressSanitizer and UBSan, and fed hex vectors on stdin; nothing is loaded into Python under a sanitizer.  What a block must
decode to is the answer of tests/lz4_model.py, which is itself pinned to liblz4 through pyarrow's codec in both directions."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pyarrow as pa
import pytest

from tests import lz4_model as M
from tests import lz4_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arrow_go_amd", "csrc")
SYMBOL = "ah_lz4_decompress_blocks"


# ---- the model against an independent implementation -----------------------------------------------------------------------------
def test_xxh32_known_values():
    assert M.xxh32(b"") == 0x02CC5D05 and M.xxh32(b"a") == 0x550D7456 and M.xxh32(b"abc") == 0x32D153FF
    assert M.xxh32(b"Nobody inspects the spammish repetition") == 0xE2293B2F


@pytest.mark.parametrize("n", [0, 1, 12, 13, 100, 65535, 65536, 65537, 3 * 65536 + 5])
def test_frames_of_the_model_inflate_through_liblz4(n):
    rng = np.random.default_rng(n)
    data = rng.integers(0, 4, n, dtype=np.uint8).tobytes()
    f = M.independent_frame(data)
    assert f[4] == 0x60 and f[5] == 0x40
    assert pa.Codec("lz4").decompress(f, decompressed_size=n).to_pybytes() == data
    assert n < 1000 or len(f) < n      # (it does compress)
    blocks = M.parse_frame(f)[2]
    assert len(blocks) == -(-n // 65536)
    # a stored block and a content-size field are read by liblz4 too
    f = M.frame([(data[:65536], True)] + M.split_blocks(data[65536:]), flg=M.FLG_VERSION | M.FLG_INDEP | M.FLG_CONTENT_SIZE, content_size=n) if n else None
    assert f is None or pa.Codec("lz4").decompress(f, decompressed_size=n).to_pybytes() == data


@pytest.mark.parametrize("n", [1, 100, 5000, 65536])
def test_the_model_decoder_inflates_what_liblz4_writes(n):
    rng = np.random.default_rng(n + 1)
    data = rng.integers(0, 3, n, dtype=np.uint8).tobytes()
    flg, bd, blocks, end = M.parse_frame(pa.Codec("lz4").compress(data).to_pybytes())   # one block: nothing to be linked to
    assert len(blocks) == 1
    assert (blocks[0][0] if blocks[0][1] else M.decode_block(blocks[0][0], n)) == data
    assert M.decode_block(pa.Codec("lz4_raw").compress(data).to_pybytes(), n) == data
    assert M.decode_block(M.compress_block(data), n) == data and M.decode_block(M.compress_block(data), n + 1) is None


# ---- the harness --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness():
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    d = tempfile.mkdtemp(prefix="lz4_harness_")
    exe = os.path.join(d, "lz4_harness")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror", "-o", exe,
                        os.path.join(ROOT, "tests", "lz4_harness.cc")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and not p.stderr, f"exit {p.returncode}\n{p.stderr[-3000:]}"
        out = p.stdout.splitlines()
        assert len(out) == len(lines)
        return out

    yield run
    shutil.rmtree(d, ignore_errors=True)


def block_line(vec, mis=0):
    name, src, stored, dst_len = vec
    return f"B {int(stored)} {dst_len} {mis} {src.hex() or '-'}"


def decoded(answer):
    status, payload = answer.split()
    return int(status), (b"" if payload == "-" else bytes.fromhex(payload))


def test_sequence_vectors(harness):
    vecs = V.sequence_vectors()
    names = " ".join(v[0] for v in vecs)
    for must in ("literals_0", "literals_14", "literals_15", "literals_270", "match_4", "match_18", "match_19", "match_600", "literals_only", "stored",
                 *(f"offset_{o}_" for o in (1, 2, 3, 7, 8, 63, 64, 65, 65535)), *(f"output_{n}_" for n in (1, 63, 64, 65, 65535, 65536))):
        assert must in names, must
    for mis in (0, 1, 15):     # where the block starts inside a 16-byte line decides which loads of the input window are whole
        for vec, answer in zip(vecs, harness([block_line(v, mis) for v in vecs])):
            status, got = decoded(answer)
            want = V.expected(vec)
            if want is None:
                assert status != 0, vec[0]
            else:
                assert status == 0 and got == want, (vec[0], mis, status)
    accepted = sum(V.expected(v) is not None for v in vecs)
    assert accepted >= len(vecs) - 4       # the vectors are, but for the named exceptions, valid blocks


def test_mutations(harness):
    """2000 seeded single-byte flips and truncations: no sanitizer report, exit 0, a status or exactly dst_len bytes, and the model's
    bytes wherever the model accepts the block"""
    vecs = V.mutation_vectors(2000)
    answers = harness([block_line(v, i % 16) for i, v in enumerate(vecs)])
    accepted = 0
    for vec, answer in zip(vecs, answers):
        status, got = decoded(answer)
        want = V.expected(vec)
        assert status in (0, 1, 2)
        assert status != 0 or len(got) == vec[3], vec[0]
        if want is not None:
            accepted += 1
            assert status == 0 and got == want, vec[0]
        else:
            assert status != 0, vec[0]
    assert 0 < accepted < len(vecs)      # flips inside literals leave a block valid: both outcomes are exercised


def test_damaged_blocks(harness):
    blocks = V.damaged_blocks()
    assert len(blocks) == 5
    for (name, (src, n)), answer in zip(blocks.items(), harness([block_line((k, s, False, n)) for k, (s, n) in blocks.items()])):
        assert M.decode_block(src, n) is None, name
        assert decoded(answer)[0] != 0, name


def test_empty_and_degenerate_blocks(harness):
    lines = ["B 0 0 0 -", "B 1 0 0 -", "B 0 5 0 -", "B 0 0 0 00", "B 0 1 3 10aa", "B 1 4 0 aabbccdd"]
    got = [decoded(a) for a in harness(lines)]
    assert got[0][0] != 0 and got[1] == (0, b"") and got[2][0] != 0 and got[3] == (0, b"") and got[4] == (0, b"\xaa") and got[5] == (0, bytes.fromhex("aabbccdd"))


# ---- the planner ----------------------------------------------------------------------------------------------------------------------
def plan(harness, cases):
    out = []
    for answer in harness([f"P {ulen} {f.hex()}" for f, ulen in cases]):
        t = [int(x) for x in answer.split()]
        out.append(None if t[0] == 0 else [tuple(t[2 + 5 * i:7 + 5 * i]) for i in range(t[1])])
    return out


def test_planner_table(harness):
    rng = np.random.default_rng(3)
    n = 2 * 65536 + 60000
    data = rng.integers(0, 4, n, dtype=np.uint8).tobytes()
    blocks = M.split_blocks(data)
    blocks[1] = (data[65536:2 * 65536], True)      # a stored block in the middle
    ok = M.frame(blocks)
    F = M.FLG_VERSION | M.FLG_INDEP
    # 65536 + 60000 + 65536 bytes: as many blocks as the length asks for, the middle one short
    short_middle = M.split_blocks(data[:65536]) + M.split_blocks(data[65536:125536]) + M.split_blocks(data[125536:])
    assert len(short_middle) == 3
    cases = {
        "qualifies": (ok, n, True),
        "qualifies with content size": (M.frame(blocks, flg=F | M.FLG_CONTENT_SIZE, content_size=n), n, True),
        "short middle block (the plan cannot see it: the decoder reports it)": (M.frame(short_middle), n, True),
        "ulen 0": (M.frame([]), 0, True),
        "bad magic": (b"\x05" + ok[1:], n, False),
        "version 00": (M.frame(blocks, flg=M.FLG_INDEP), n, False),
        "version 10": (M.frame(blocks, flg=0x80 | M.FLG_INDEP), n, False),
        "linked blocks": (M.frame(blocks, flg=M.FLG_VERSION), n, False),
        "block checksums": (M.frame(blocks, flg=F | M.FLG_BLOCK_CHECKSUM), n, False),
        "content checksum": (M.frame(blocks, flg=F | M.FLG_CONTENT_CHECKSUM, content=data), n, False),
        "DictID": (M.frame(blocks, flg=F | M.FLG_DICT_ID, dict_id=7), n, False),
        "reserved FLG bit": (M.frame(blocks, flg=F | M.FLG_RESERVED), n, False),
        "reserved BD bit": (ok[:5] + bytes([0x41, (M.xxh32(bytes([ok[4], 0x41])) >> 8) & 0xFF]) + ok[7:], n, False),
        "BD code 5": (M.frame(blocks, bd_code=5), n, False),
        "BD code 7": (M.frame(blocks, bd_code=7), n, False),
        "header checksum": (M.frame(blocks, header_checksum=(ok[6] + 1) & 0xFF), n, False),
        "content size differs": (M.frame(blocks, flg=F | M.FLG_CONTENT_SIZE, content_size=n + 1), n, False),
        "announced length differs: a block too many": (ok, n - 65536, False),
        "announced length differs: a block missing": (ok, n + 65536, False),
        "no EndMark": (ok[:-4], n, False),
        "trailing bytes after the EndMark": (M.frame(blocks, trailing=b"\0\0\0\0"), n, False),
        "one trailing byte": (M.frame(blocks, trailing=b"\x01"), n, False),
        "block runs past the frame": (ok[:-40], n, False),
        "stored size beyond 64 KiB": (M.frame([(bytes(65537), True)]), 65537, False),
        "blocks but ulen 0": (M.frame(blocks[:1]), 0, False),
        "truncated header": (ok[:6], n, False),
        "empty": (b"", 0, False),
    }
    plans = plan(harness, [(f, u) for f, u, _ in cases.values()])
    for (name, (f, u, want)), got in zip(cases.items(), plans):
        assert (got is not None) == want, name
    # the plan of the qualifying frame, block by block
    got, at, expect = plans[0], 7, []
    for i, (b, stored) in enumerate(blocks):
        expect.append((at + 4, len(b), 65536 * i, min(65536, n - 65536 * i), int(stored)))
        at += 4 + len(b)
    assert got == expect and plans[3] == []
    assert [p[3] for p in plans[2]] == [65536, 65536, 60000]    # every block but the last is taken for 64 KiB
    # liblz4 agrees that the qualifying frames are frames of `data`
    assert pa.Codec("lz4").decompress(ok, decompressed_size=n).to_pybytes() == data
    assert pa.Codec("lz4").decompress(M.frame(short_middle), decompressed_size=n).to_pybytes() == data


# ---- build and ABI ----------------------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    from arrow_go_amd import _native as N
    from arrow_go_amd import device as D
    from arrow_go_amd import compute as ac
    out = subprocess.check_output(["nm", "-D", "--defined-only", N.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert SYMBOL in N.declared_symbols() and SYMBOL in exported
    assert getattr(N.lib, SYMBOL).argtypes is not None and len(getattr(N.lib, SYMBOL).argtypes) == 9
    assert callable(D.Context.lz4_decompress_blocks)
    assert "lib." + SYMBOL in open(os.path.join(ROOT, "arrow_go_amd", "device.py")).read()
    assert "C." + SYMBOL + "(" in open(os.path.join(ROOT, "go", "arrowhip", "extra.go")).read()
    assert ac.lib.ahc_ipc_stats.argtypes is not None
    assert "ahc_ipc_stats" in open(os.path.join(ROOT, "include", "arrowhip_compute.h")).read()


def test_kernel_has_no_scratch_and_the_lds_the_design_states():
    """ah_lz4.hip compiles for gfx950 with zero scratch bytes; its group segment is the 64 KiB image + 4 KiB window of DESIGN.md §3.8 —
    two blocks per CU under gfx950's 160 KiB (read from the ISA the way tests/test_hash_min_max.py reads it)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the library under test cannot have been built without it"
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "lz4.s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-S",
                            "--cuda-device-only", "-o", out, os.path.join(CSRC, "ah_lz4.hip")], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(out).read()
    kernels = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        p = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
        g = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", m.group(2))
        kernels[m.group(1)] = (int(p.group(1)), int(g.group(1)))
    assert len(kernels) == 1 and "lz4_blocks_kernel" in next(iter(kernels))
    scratch, lds = next(iter(kernels.values()))
    assert scratch == 0, f"{scratch} bytes of scratch"
    assert lds == 65536 + 4096 and 2 * lds <= 163840
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "69 632 B" in design or "69632" in design
