"""Byte-level host model of the string predicates: the yardstick of ah_string_match / _find / _like / _length and of
the registry functions above them.  Python `bytes` operations and a small LIKE matcher (the textbook recursion over pattern tokens,
evaluated backwards), written without a look at the device's segment program.  Like the C ABI, every row is computed, null slots included: validity is the caller's.

A column is a list of `bytes` rows.  rows_of() cuts one out of Arrow buffers (offsets, data, array offset)."""
import numpy as np


def rows_of(offsets, data, off, n):
    o = np.asarray(offsets)
    d = bytes(np.asarray(data, np.uint8).tobytes())
    return [d[int(o[off + i]):int(o[off + i + 1])] for i in range(n)]


def match_substring(rows, pattern):
    return np.array([pattern in r for r in rows], bool)


def starts_with(rows, pattern):
    return np.array([r.startswith(pattern) for r in rows], bool)


def ends_with(rows, pattern):
    return np.array([r.endswith(pattern) for r in rows], bool)


def equals(rows, pattern):
    return np.array([r == pattern for r in rows], bool)


def find_substring(rows, pattern, dtype=np.int32):
    return np.array([r.find(pattern) for r in rows], dtype)


def binary_length(rows, dtype=np.int32):
    return np.array([len(r) for r in rows], dtype)


def utf8_length(rows, dtype=np.int32):
    """code points = bytes that are not 10xxxxxx continuation bytes (the rule also on bytes that are no valid UTF-8)"""
    return np.array([sum(1 for b in r if b & 0xC0 != 0x80) for r in rows], dtype)


def _tokens(pattern):
    """the LIKE pattern as tokens: ('%',), ('_',), ('lit', byte); a lone escape character at the end is dropped, as Arrow drops it"""
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i]
        if c == 0x5C:   # backslash: the next pattern character is literal, whatever it is
            if i + 1 == len(pattern):
                break
            out.append(("lit", pattern[i + 1]))
            i += 2
            continue
        out.append(("%",) if c == 0x25 else ("_",) if c == 0x5F else ("lit", c))
        i += 1
    return out


def _one_char(row, x, utf8):
    """the position behind the one character `_` takes at x, or None"""
    if x >= len(row):
        return None
    if not utf8:
        return x + 1
    if row[x] & 0xC0 == 0x80:
        return None
    x += 1
    while x < len(row) and row[x] & 0xC0 == 0x80:
        x += 1
    return x


def like_row(row, tokens, utf8):
    """The whole row against the tokens.  The recursion  match(t, x) = tokens[t:] match row[x:]  — `%`: some y >= x with
    match(t + 1, y); `_`: match(t + 1, behind the character at x); a literal: row[x] is it and match(t + 1, x + 1) — evaluated
    from the last token backwards for all x at once (a row of tens of thousands of bytes would overflow the interpreter's stack)."""
    b = np.frombuffer(row, np.uint8)
    n = len(b)
    ok = np.zeros(n + 1, bool)
    ok[n] = True   # behind the last token: the row must be used up
    if utf8:
        lead = (b & 0xC0) != 0x80
        starts = np.where(np.append(lead, True), np.arange(n + 1), n)        # x where a character (or the end) starts, else n
        behind = np.minimum.accumulate(starts[::-1])[::-1][1:]                # behind[x]: the first such position after x
    for tok in reversed(tokens):
        new = np.zeros(n + 1, bool)
        if tok[0] == "%":
            new = np.logical_or.accumulate(ok[::-1])[::-1]
        elif tok[0] == "_":
            if utf8:
                new[:n] = lead & ok[behind]
            else:
                new[:n] = ok[1:]
        else:
            new[:n] = (b == tok[1]) & ok[1:]
        ok = new
    return bool(ok[0])


def match_like(rows, pattern, utf8):
    """Arrow C++'s match_like as pyarrow 25 answers.  Arrow first tries three shortcuts by regular expression over the pattern and
    hands what they capture to its substring / prefix / suffix matchers RAW, escape characters included (`%a\\bc%` finds `a\\bc`);
    only the patterns that miss all three have their escapes resolved."""
    import re
    for shape, fn in ((rb"%+([^%_]*[^\\%_])?%+", match_substring), (rb"([^%_]*[^\\%_])?%+", starts_with), (rb"%+([^%_]*)", ends_with)):
        m = re.fullmatch(shape, pattern, re.S)
        if m:
            return fn(rows, m.group(1) or b"")
    tokens = _tokens(pattern)
    return np.array([like_row(r, tokens, utf8) for r in rows], bool)


def run_program(program, row, utf8):
    """A small interpreter of the compiled LIKE program (include/arrowhip.h) for the host tests: segments tried at EVERY position by
    backtracking — not leftmost-greedy like the device — so that it also checks that greedy loses nothing."""
    flags, nseg = program[0], program[1] | (program[2] << 8)
    segs, at = [], 3
    for _ in range(nseg):
        ne = program[at] | (program[at + 1] << 8)
        segs.append([(program[at + 2 + 2 * e], program[at + 3 + 2 * e]) for e in range(ne)])
        at += 2 + 2 * ne
    assert at == len(program), "bytes behind the last segment"

    def seg_at(seg, x):
        for kind, b in seg:
            if kind == 0:
                if x >= len(row) or row[x] != b:
                    return None
                x += 1
            else:
                x = _one_char(row, x, utf8)
                if x is None:
                    return None
        return x

    def go(s, x, free):
        """segments s … from position x; free: a `%` stands in front of segment s"""
        if s == len(segs):
            return x == len(row) or not (flags & 2)
        starts = range(x, len(row) + 1) if free else [x]
        for y in starts:
            e = seg_at(segs[s], y)
            if e is not None and go(s + 1, e, True):
                return True
        return False

    if nseg == 0:
        return True
    return go(0, 0, not (flags & 1))


def pack(flags, off=0, prev=None):
    """the flags at bits off … of a bitmap (LSB first) whose other bits are `prev`'s"""
    nbytes = (off + len(flags) + 7) // 8
    bits = np.zeros(nbytes * 8, bool) if prev is None else np.unpackbits(np.asarray(prev, np.uint8)[:nbytes], bitorder="little").astype(bool)
    bits[off:off + len(flags)] = flags
    return np.packbits(bits, bitorder="little")
