"""Block vectors shared by tests/test_lz4_host.py (the host harness under sanitizers) and tests/test_ipc_lz4_device.py (the same
blocks on the GPU): hand-assembled sequences, the seeded mutations, and the damaged blocks.  A vector is (name, block bytes, stored,
dst_len); what it must decode to is always tests/lz4_model.decode_block's answer (None: a non-zero status)."""
import numpy as np

from tests import lz4_model as M


def _bytes(rng, n, alphabet=256):
    return rng.integers(0, alphabet, n, dtype=np.uint8).tobytes()


def expected(vec):
    name, src, stored, dst_len = vec
    if stored:
        return bytes(src) if len(src) == dst_len else None
    return M.decode_block(src, dst_len)


def sequence_vectors():
    """literal lengths 0 / 14 / 15 / 15 + 255, match lengths 4 / 18 / 19 / >= 600, offsets 1, 2, 3, 7, 8, 63, 64, 65, 65535 (an
    independent block of <= 64 KiB has no room for a match 65535 back — 65535 + 4 bytes —, so that vector must be refused, and 65532,
    the farthest offset that fits, stands beside it), a block of literals only, a stored block, outputs of 1, 63, 64, 65, 65535 and
    65536 bytes."""
    rng = np.random.default_rng(20260)
    out = []

    def add(name, seqs, dst_len=None):
        src = b"".join(M.sequence(*s) for s in seqs)
        if dst_len is None:
            dst_len = sum(len(s[0]) + (s[2] if len(s) > 1 else 0) for s in seqs)
        out.append((name, src, False, dst_len))

    for ll in (0, 14, 15, 270):   # the literal run under test is the SECOND sequence's; the first provides bytes to match
        add(f"literals_{ll}", [(_bytes(rng, 9), 4, 5), (_bytes(rng, ll), 3, 7), (_bytes(rng, 5),)])
    for ml in (4, 18, 19, 600, 1000):
        add(f"match_{ml}", [(_bytes(rng, 40), 33, ml), (_bytes(rng, 6),)])
    for off in (1, 2, 3, 7, 8, 63, 64, 65):
        for ml in (4, 70, 300):      # shorter than, around and far beyond the offset: the match runs into its own output
            add(f"offset_{off}_match_{ml}", [(_bytes(rng, off + 2), off, ml), (_bytes(rng, 5),)])
    add("offset_65532_last_that_fits", [(_bytes(rng, 65532), 65532, 4), (b"",)])
    add("offset_65535_cannot_fit", [(_bytes(rng, 65535), 65535, 4), (b"",)], dst_len=65536)
    add("offset_65535_before_the_block", [(_bytes(rng, 100), 65535, 4), (_bytes(rng, 5),)])
    add("literals_only", [(_bytes(rng, 333),)])
    add("two_matches_back_to_back", [(_bytes(rng, 20), 20, 20), (b"", 7, 9), (b"", 1, 64), (_bytes(rng, 5),)])
    out.append(("stored", _bytes(rng, 777), True, 777))
    out.append(("stored_wrong_size", _bytes(rng, 100), True, 101))
    for n in (1, 63, 64, 65, 65535, 65536):
        data = _bytes(rng, n, alphabet=4)
        out.append((f"output_{n}_compressed", M.compress_block(data), False, n))
        out.append((f"output_{n}_stored", data, True, n))
    long_zero = bytes(65536)
    out.append(("output_65536_one_long_match", M.compress_block(long_zero), False, 65536))
    return out


def mutation_vectors(count=2000, seed=7):
    """seeded single-byte flips and truncations of valid blocks of 40 … 1500 output bytes"""
    rng = np.random.default_rng(seed)
    bases = []
    for k in range(40):
        n = int(rng.integers(40, 1500))
        data = _bytes(rng, n, alphabet=int(rng.choice([2, 4, 16, 256])))
        if k % 4 == 0:                      # long runs: length-extension bytes to flip
            data = data[:20] + bytes([data[0]]) * (n - 20)
        bases.append((M.compress_block(data), n))
    out = []
    for i in range(count):
        src, n = bases[i % len(bases)]
        b = bytearray(src)
        if i % 5 == 4:
            b = b[:int(rng.integers(0, len(b)))]
        else:
            at = int(rng.integers(0, len(b)))
            b[at] ^= int(rng.integers(1, 256))
        out.append((f"mutation_{i}", bytes(b), False, n))
    return out


def damaged_blocks():
    """five blocks that are wrong in one way each; every one must come back with a status: name → (block, dst_len)"""
    lit = bytes(range(16))
    return {
        "offset_before_block_start": (M.sequence(lit[:8], 9, 8) + M.sequence(lit[:5]), 21),
        "offset_zero": (M.sequence(lit[:8], 0, 8) + M.sequence(lit[:5]), 21),
        "literal_run_past_source_end": (bytes([0xF0, 200]) + lit, 215),
        "output_overrun": (M.sequence(lit[:8], 4, 600) + M.sequence(lit[:5]), 100),
        "token_at_last_byte": (M.sequence(lit[:8], 4, 8) + bytes([0x50]), 21),
    }
