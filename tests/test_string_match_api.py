"""match_substring, starts_with, ends_with, find_substring, match_like, binary_length and utf8_length through Session against pyarrow
(Arrow C++ defines them): the four binary-like types, nulls, sliced inputs (array offset 5, a first offset that is not 0, validity
at a bit offset), chunked inputs with an empty chunk, a keep_on_device mask chained into filter, and two tile sizes.  Results are
compared with Array.equals: every expected value is exact."""
import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc  # noqa: E402

pytestmark = pytest.mark.gpu

TYPES = [pa.string(), pa.binary(), pa.large_string(), pa.large_binary()]
PIECES = ["a", "b", "ab", "c", "é", "日", "\n", "%", "_", "BRASS", " "]


@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.set_option("string_tile_bytes", 0)
    s.close()


def column(t, n, seed, null_rate=0.15, offset=5, max_pieces=12):
    rng = np.random.default_rng(seed)
    total = n + offset
    vals = ["".join(rng.choice(PIECES, int(k))) for k in rng.integers(0, max_pieces + 1, total)]
    if total > 40:
        vals[offset + 7] = "x" * 3000 + "PROMO BRASS"     # a row of several small tiles
    if pa.types.is_binary(t) or pa.types.is_large_binary(t):
        vals = [v.encode() for v in vals]
    mask = rng.random(total) < null_rate
    return pa.array([None if m else v for v, m in zip(vals, mask)], type=t).slice(offset, n)


def same(got, want):
    if isinstance(want, pa.ChunkedArray):
        assert isinstance(got, pa.ChunkedArray) and [len(c) for c in got.chunks] == [len(c) for c in want.chunks]
        for g, w in zip(got.chunks, want.chunks):
            same(g, w)
        return
    assert got.type == want.type and len(got) == len(want), (got.type, want.type, len(got), len(want))
    got.validate(full=True)
    assert got.equals(want), [(i, g, w) for i, (g, w) in enumerate(zip(got.to_pylist(), want.to_pylist())) if g != w][:5]


def every_function(sess, arr):
    """(name, ours, pyarrow's) for every function the type takes"""
    out = []
    for pat in ("ab", "", "BRASS", "é", "b\nc"):
        out.append(("match_substring " + pat, sess.match_substring(arr, pat), pc.match_substring(arr, pat)))
        out.append(("starts_with " + pat, sess.starts_with(arr, pat), pc.starts_with(arr, pat)))
        out.append(("ends_with " + pat, sess.ends_with(arr, pat), pc.ends_with(arr, pat)))
        out.append(("find_substring " + pat, sess.find_substring(arr, pat), pc.find_substring(arr, pat)))
    for pat in ("%BRASS", "%a%b%", "a_%", "_", "%é_", "ab", "%", "a\\%%", "%PROMO%BRASS", "_b%\n%"):
        out.append(("match_like " + pat, sess.match_like(arr, pat), pc.match_like(arr, pat)))
    out.append(("binary_length", sess.binary_length(arr), pc.binary_length(arr)))
    if "string" in str(arr.type):
        out.append(("utf8_length", sess.utf8_length(arr), pc.utf8_length(arr)))
    return out


@pytest.mark.parametrize("t", TYPES, ids=str)
@pytest.mark.parametrize("tile", [0, 256])
def test_every_function_is_pyarrows(sess, t, tile):
    sess.set_option("string_tile_bytes", tile)
    arr = column(t, 2000, seed=len(str(t)))
    assert arr.offset == 5 and arr.null_count > 0
    for name, got, want in every_function(sess, arr):
        same(got, want)


def test_bytes_patterns_and_no_nulls(sess):
    sess.set_option("string_tile_bytes", 0)
    arr = pa.array([b"h\xffllo", b"hello", b"", b"\xff", b"a;b=c"], type=pa.binary())
    same(sess.match_substring(arr, b"\xff"), pc.match_substring(arr, b"\xff"))
    same(sess.find_substring(arr, b";b="), pc.find_substring(arr, b";b="))
    same(sess.match_like(arr, b"h_llo"), pc.match_like(arr, b"h_llo"))
    same(sess.match_like(pa.array(["héllo\nx", "h_llo"]), "h_llo%"), pa.array([True, True]))
    fixed = pa.array([b"abc", None, b"xyz"], type=pa.binary(3))
    same(sess.binary_length(fixed), pc.binary_length(fixed))
    same(sess.binary_length(fixed.slice(1, 2)), pc.binary_length(fixed.slice(1, 2)))


@pytest.mark.parametrize("t", [pa.string(), pa.large_binary()], ids=str)
def test_chunked_input_with_an_empty_chunk(sess, t):
    """one output chunk per non-empty input chunk: the rule of every chunked call"""
    sess.set_option("string_tile_bytes", 256)
    parts = [column(t, 300, 1), column(t, 0, 2), column(t, 65, 3), column(t, 1, 4)]
    ch = pa.chunked_array(parts)
    for name, got, want in every_function(sess, ch):
        assert isinstance(got, pa.ChunkedArray), name
        assert [len(c) for c in got.chunks] == [300, 65, 1], name
        same(got.combine_chunks(), want.combine_chunks())


def test_results_do_not_depend_on_the_tile(sess):
    arr = column(pa.string(), 5000, seed=9)
    results = {}
    for tile in (0, 64, 333, 4096):
        sess.set_option("string_tile_bytes", tile)
        results[tile] = [got for _, got, _ in every_function(sess, arr)]
    for tile in (64, 333, 4096):
        for a, b in zip(results[0], results[tile]):
            same(b, a)


def test_a_like_mask_stays_on_the_device_for_filter(sess):
    """WHERE name LIKE '%BRASS' in front of a filter: the mask never leaves HBM"""
    sess.set_option("string_tile_bytes", 0)
    rng = np.random.default_rng(5)
    names = column(pa.string(), 4000, seed=6)
    price = pa.array(rng.integers(0, 1000, 4000), type=pa.int64())
    mask = sess.match_like(names, "%BRASS", keep_on_device=True)
    want_mask = pc.match_like(names, "%BRASS")
    same(sess.call_function("filter", [price, mask]), pc.filter(price, want_mask))
    same(sess.call_function("filter", [names, mask]), pc.filter(names, want_mask))
    both = sess.call_function("and", [mask, sess.starts_with(names, "a", keep_on_device=True)], keep_on_device=True)
    same(sess.call_function("filter", [price, both]), pc.filter(price, pc.and_(want_mask, pc.starts_with(names, "a"))))


def test_refusals(sess):
    from arrow_go_amd import compute as ac
    arr = pa.array(["a", "b"])
    with pytest.raises(ac.ErrNotImplemented, match="ignore_case=true is not implemented"):
        sess.match_substring(arr, "a", ignore_case=True)
    with pytest.raises(ac.ErrInvalid, match="needs the option pattern_hex"):
        sess.call_function("match_like", [arr])
    with pytest.raises(ac.ErrInvalid, match="pattern_hex is not a string of hex byte pairs"):
        sess.call_function("starts_with", [arr], "pattern_hex=zz")
    with pytest.raises(ac.ErrNotImplemented, match=r"function 'utf8_length' has no kernel matching input types \(binary\)"):
        sess.utf8_length(pa.array([b"a"], type=pa.binary()))
    with pytest.raises(ac.ErrNotImplemented, match=r"function 'match_substring' has no kernel matching input types \(int32\)"):
        sess.match_substring(pa.array([1, 2], type=pa.int32()), "a")
    for call in (lambda: sess.match_substring(pa.scalar("abc"), "a"), lambda: sess.utf8_length(pa.scalar("abc"))):
        with pytest.raises(ac.ErrNotImplemented, match="takes an array or a chunked array, not a scalar"):   # no function takes a scalar input
            call()
