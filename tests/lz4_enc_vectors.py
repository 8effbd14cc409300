"""Input blocks for the LZ4 block compressor (csrc/ah_lz4_enc.h), shared by its host test (tests/test_lz4_enc_host.py) and its device
test (tests/test_ipc_writer.py), with a parser of the sequences of a compressed block that checks the encoder-side rules of
lz4_Block_format.md.  Every vector is (name, bytes); the contents are functions of fixed seeds."""
import functools

import numpy as np

BLOCK = 65536
LENGTHS = (0, 1, 4, 12, 13, 14, 63, 64, 65, 4095, 4096, 65535, 65536)


def _rng(*key):
    return np.random.default_rng([17, *key])


def _random(n, *key, alphabet=256):
    return _rng(*key).integers(0, alphabet, n, dtype=np.uint8).tobytes()


def _periodic(period, n):
    return (_random(period, 1, period) * (n // period + 1))[:n]


def planted_match(length, seed=0):
    """random bytes | a copy of `length` of them, cut off by a byte that differs | random bytes: one match of exactly `length`"""
    head = _random(400, 2, length, seed)
    at = 37
    breaker = bytes([head[at + length] ^ 0x55])
    return head + head[at:at + length] + breaker + _random(40, 3, length, seed)


def planted_literals(run, seed=0):
    """pattern | pattern | `run` random bytes | pattern | random tail: the third pattern's sequence carries exactly `run` literals"""
    pat = _random(96, 4, run, seed)
    return pat + pat + _random(run, 5, run, seed) + pat + _random(40, 6, run, seed)


@functools.lru_cache(maxsize=None)
def vectors():
    out = []
    for n in LENGTHS:
        out.append((f"zeros_{n}", bytes(n)))
        out.append((f"alphabet4_{n}", _random(n, 7, n, alphabet=4)))
        out.append((f"text_{n}", (b"the quick brown fox jumps over the lazy dog; " * (n // 45 + 1))[:n]))
    for period in (1, 3, 64, 65, 4097):
        out.append((f"period_{period}", _periodic(period, 3 * 4097 + 11)))
        out.append((f"period_{period}_full", _periodic(period, BLOCK)))
    body = _random(60, 8)
    out.append(("match_into_the_last_12", body + body))                             # the repeat runs to the very end
    out.append(("match_ends_5_before_the_end", body + body[:30] + bytes([body[30] ^ 1, 1, 2, 3, 4])))
    for length in (18, 19, 273, 274):
        out.append((f"match_len_{length}", planted_match(length)))
    for run in (14, 15, 270):
        out.append((f"literal_run_{run}", planted_literals(run)))
    out.append(("uniform_random", _random(BLOCK, 9)))
    out.append(("uniform_random_1000", _random(1000, 9, 1)))
    out.append(("alphabet4_mixed", b"".join(_random(3000, 10, k, alphabet=256 if k % 2 else 3) for k in range(9))))
    out.append(("int64_counter", np.arange(10**6, 10**6 + BLOCK // 8, dtype=np.int64).tobytes()))
    words = [b"alpha", b"beta", b"gamma-ray", b"delta", b"epsilon", b"zeta", b"eta"]
    picks = _rng(11).integers(0, len(words), 16000)
    out.append(("string_data", b"".join(words[k] for k in picks)[:BLOCK]))
    return tuple(out)


def parse_sequences(block, n):
    """[(literal length, offset or None, match length or None, output position of the match)] of a block that inflates to n bytes;
    asserts the encoder-side rules: offsets 1 … position, the last sequence has no match and at least 5 literals, the last match
    starts at least 12 bytes before the end, a block under 13 bytes is literals only"""
    seqs, sp, op = [], 0, 0
    while True:
        token = block[sp]
        sp += 1
        ll = token >> 4
        if ll == 15:
            while True:
                b = block[sp]
                sp += 1
                ll += b
                if b != 255:
                    break
        sp += ll
        op += ll
        assert sp <= len(block) and op <= n
        if sp == len(block):
            seqs.append((ll, None, None, op))
            break
        offset = block[sp] | (block[sp + 1] << 8)
        sp += 2
        assert 1 <= offset <= op, f"offset {offset} at output position {op}"
        ml = token & 15
        if ml == 15:
            while True:
                b = block[sp]
                sp += 1
                ml += b
                if b != 255:
                    break
        ml += 4
        seqs.append((ll, offset, ml, op))
        op += ml
    assert op == n
    matches = [s for s in seqs if s[1] is not None]
    if matches:
        assert n >= 13
        assert seqs[-1][0] >= 5, "the last five bytes are literals"
        assert matches[-1][3] <= n - 12, "the last match starts at least 12 bytes before the end"
        assert all(s[3] + s[2] <= n - 5 for s in matches)
    return seqs
