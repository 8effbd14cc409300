"""ascii_upper / ascii_lower, utf8_slice_codeunits, binary_slice and the nine trims through Session against pyarrow (Arrow C++ defines
them): arrays with and without nulls, sliced arrays (array offset 5, a first offset that is not 0, validity at a bit offset), chunked
arrays with an empty chunk, the Large types, a column imported through import_host (uploaded at import: strings are never host-resident), a chain that stays on the device, and the refusals.  Results are
compared with Array.equals after validate(full=True); the output's validity and null count are the input's."""
import ctypes as C

import numpy as np
import pytest

pa = pytest.importorskip("pyarrow")
import pyarrow.compute as pc  # noqa: E402

pytestmark = pytest.mark.gpu

STRING_TYPES = [pa.string(), pa.large_string()]
BINARY_TYPES = [pa.binary(), pa.large_binary()]
PIECES = ["a", "B", "ab", " ", "  ", "é", "€", "𝄞", "\t", "x", "Zz", "BRASS"]


@pytest.fixture(scope="module")
def sess():
    from arrow_go_amd import compute as ac
    s = ac.Session(0)
    yield s
    s.set_option("string_tile_bytes", 0)
    s.close()


def column(t, n, seed, null_rate=0.15, offset=5, max_pieces=10):
    rng = np.random.default_rng(seed)
    total = n + offset
    vals = ["".join(rng.choice(PIECES, int(k))) for k in rng.integers(0, max_pieces + 1, total)]
    if total > 40:
        vals[offset + 7] = " " * 70 + "x" * 6000 + "é" * 40 + " \t"     # a row the wave walks and the workgroup copies
    if t in BINARY_TYPES:
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
    assert got.null_count == want.null_count
    assert got.is_valid().equals(want.is_valid())
    assert got.equals(want), [(i, g, w) for i, (g, w) in enumerate(zip(got.to_pylist(), want.to_pylist())) if g != w][:5]


def every_function(sess, arr):
    """(name, ours, pyarrow's) for every function the type takes"""
    out = []
    if arr.type in BINARY_TYPES:
        for start, stop in ((0, 2), (2, None), (-4, None), (1, -1), (-100, 3), (5, 2), (0, None)):
            # (pyarrow 25's binary_slice reserves rows × (stop − start) bytes and overflows on an absent stop behind a start ≥ 0: it gets a stop beyond every row)
            pa_stop = 8192 if stop is None and start >= 0 else stop
            out.append((f"binary_slice {start}:{stop}", sess.binary_slice(arr, start, stop), pc.binary_slice(arr, start, pa_stop)))
        return out
    out.append(("ascii_upper", sess.ascii_upper(arr), pc.ascii_upper(arr)))
    out.append(("ascii_lower", sess.ascii_lower(arr), pc.ascii_lower(arr)))
    for start, stop in ((0, 2), (2, None), (-4, None), (1, -1), (-100, 3), (5, 2), (0, None), (75, 6080), (-45, -3)):
        out.append((f"utf8_slice_codeunits {start}:{stop}", sess.utf8_slice_codeunits(arr, start, stop), pc.utf8_slice_codeunits(arr, start, stop)))
    for side in ("trim", "ltrim", "rtrim"):
        name = f"ascii_{side}_whitespace"
        out.append((name, getattr(sess, name)(arr), getattr(pc, name)(arr)))
        for chars in ("", " ", "a ", "é \t", "€𝄞xB "):
            for family in ("ascii", "utf8"):
                name = f"{family}_{side}"
                out.append((f"{name} {chars!r}", getattr(sess, name)(arr, chars), getattr(pc, name)(arr, chars)))
    return out


@pytest.mark.parametrize("t", STRING_TYPES + BINARY_TYPES, ids=str)
@pytest.mark.parametrize("tile", [0, 333])
def test_every_function_is_pyarrows(sess, t, tile):
    sess.set_option("string_tile_bytes", tile)
    arr = column(t, 2000, seed=len(str(t)))
    assert arr.offset == 5 and arr.null_count > 0
    for name, got, want in every_function(sess, arr):
        same(got, want)
    plain = column(t, 500, seed=3, null_rate=0.0, offset=0)
    assert plain.null_count == 0
    for name, got, want in every_function(sess, plain):
        same(got, want)


def test_offsets_under_nulls_and_the_issues_examples(sess):
    sess.set_option("string_tile_bytes", 0)
    got = sess.ascii_trim(pa.array(["xx", None, "ax"]), "x")
    assert np.frombuffer(got.buffers()[1], np.int32)[:4].tolist() == [0, 0, 0, 1] and got.null_count == 1
    s = pa.array(["héllo wörld", "ab"])
    assert sess.utf8_slice_codeunits(s, -3, -1).to_pylist() == ["rl", "a"]
    assert sess.utf8_slice_codeunits(s, -100, 2).to_pylist() == ["hé", "ab"]
    assert sess.utf8_slice_codeunits(s, 3, 1).to_pylist() == ["", ""]
    assert sess.utf8_slice_codeunits(s, 2, 100).to_pylist() == ["llo wörld", ""]
    assert sess.utf8_trim(s, "hé d").to_pylist() == ["llo wörl", "ab"]
    assert sess.ascii_upper(pa.array(["héllo"])).to_pylist() == ["HéLLO"]
    nulls = pa.array([None, None, None], pa.large_string())
    same(sess.ascii_lower(nulls), nulls)


@pytest.mark.parametrize("t", [pa.string(), pa.large_string(), pa.large_binary()], ids=str)
def test_chunked_input_with_an_empty_chunk(sess, t):
    """one output chunk per non-empty input chunk: the rule of every chunked call"""
    sess.set_option("string_tile_bytes", 64)
    parts = [column(t, 300, 1), column(t, 0, 2), column(t, 65, 3), column(t, 1, 4)]
    ch = pa.chunked_array(parts)
    for name, got, want in every_function(sess, ch):
        assert isinstance(got, pa.ChunkedArray), name
        assert [len(c) for c in got.chunks] == [300, 65, 1], name
        same(got.combine_chunks(), want.combine_chunks())
    empty = pa.array([], t)
    for name, got, want in every_function(sess, empty):
        same(got, want)


def test_results_do_not_depend_on_the_tile(sess):
    arr = column(pa.string(), 5000, seed=9)
    results = {}
    for tile in (0, 64, 333, 4096):
        sess.set_option("string_tile_bytes", tile)
        results[tile] = [got for _, got, _ in every_function(sess, arr)]
    for tile in (64, 333, 4096):
        for a, b in zip(results[0], results[tile]):
            same(b, a)


def test_a_chain_stays_on_the_device(sess):
    """WHERE name LIKE '%BRASS%' … GROUP BY SUBSTR(name, 1, 2): mask, filtered columns and the sliced key never leave HBM"""
    from arrow_go_amd import compute as ac
    sess.set_option("string_tile_bytes", 0)
    rng = np.random.default_rng(5)
    names = column(pa.string(), 4000, seed=6)
    price = pa.array(rng.integers(0, 1000, 4000), type=pa.int64())
    mask = sess.match_like(names, "%BRASS%", keep_on_device=True)
    kept_names = sess.call_function("filter", [names, mask], keep_on_device=True)
    kept_price = sess.call_function("filter", [price, mask], keep_on_device=True)
    key = sess.utf8_slice_codeunits(kept_names, 0, 2, keep_on_device=True)
    d = C.c_void_p()
    sess._check(ac.lib.ahc_record_from_arrays(sess.h, 2, (C.c_char_p * 2)(b"k", b"v"), (C.c_void_p * 2)(key.h, kept_price.h), C.byref(d)))
    batch = ac.DeviceArray(sess, d)
    got = sess.group_by(batch, "k", [("v", "sum"), ("v", "count")])
    want_mask = pc.match_like(names, "%BRASS%")
    want_key = pc.utf8_slice_codeunits(pc.filter(names, want_mask), 0, 2)
    assert want_key.null_count == 0 and len(want_key) > 50
    same(key.to_arrow(), want_key)
    want = pa.table({"k": want_key, "v": pc.filter(price, want_mask)}).group_by("k", use_threads=False).aggregate([("v", "sum"), ("v", "count")])
    got_rows = sorted(zip(got.column("k").to_pylist(), got.column("v_sum").to_pylist(), got.column("v_count").to_pylist()))
    want_rows = sorted(zip(want.column("k").to_pylist(), want.column("v_sum").to_pylist(), want.column("v_count").to_pylist()))
    assert got_rows == want_rows and len(got_rows) > 3
    for x in (batch, key, kept_price, kept_names, mask):
        x.release()


def test_a_column_imported_as_host_resident_is_on_the_device(sess):
    """Only flat fixed-width columns can stay in host memory here: import_host uploads a string column whole at import, as the plain
    import does, so the transforms never meet a host-resident argument.  What is checked is exactly that: the import is not on the
    host, and the call is the plain call."""
    sess.set_option("host_threshold_bytes", 0)
    try:
        arr = column(pa.string(), 3000, seed=12)
        h = sess.import_host(arr)
        assert not h.on_host()
        got = sess.call_function("ascii_trim_whitespace", [h], keep_on_device=True)
        assert not got.on_host()
        same(got.to_arrow(), pc.ascii_trim_whitespace(arr))
        same(sess.utf8_slice_codeunits(h, 1, 4), pc.utf8_slice_codeunits(arr, 1, 4))
        got.release()
        h.release()
    finally:
        sess.set_option("host_threshold_bytes", 0)


def test_refusals(sess):
    from arrow_go_amd import compute as ac
    arr = pa.array(["a", "b"])
    with pytest.raises(ac.ErrNotImplemented, match="step=-1 is not implemented"):
        sess.utf8_slice_codeunits(arr, 0, None, step=-1)
    with pytest.raises(ac.ErrNotImplemented, match="step=2 is not implemented"):
        sess.binary_slice(pa.array([b"ab"]), 0, None, step=2)
    with pytest.raises(ac.ErrInvalid, match="needs the option start"):
        sess.call_function("utf8_slice_codeunits", [arr])
    with pytest.raises(ac.ErrInvalid, match="needs the option characters_hex"):
        sess.call_function("utf8_trim", [arr])
    with pytest.raises(ac.ErrInvalid, match="the characters are not valid UTF-8"):
        sess.utf8_rtrim(arr, b"\xff")
    same(sess.ascii_rtrim(arr, b"\xffb"), pa.array(["a", ""]))   # a set of bytes takes any bytes
    for name in ("ascii_upper", "utf8_trim", "utf8_slice_codeunits"):
        with pytest.raises(ac.ErrNotImplemented, match=rf"function '{name}' has no kernel matching input types \(binary\)"):
            sess.call_function(name, [pa.array([b"a"], type=pa.binary())], "start=0;characters_hex=61")
    with pytest.raises(ac.ErrNotImplemented, match=r"function 'binary_slice' has no kernel matching input types \(utf8\)"):
        sess.binary_slice(arr, 0)
    with pytest.raises(ac.ErrNotImplemented, match=r"function 'binary_slice' has no kernel matching input types"):
        sess.binary_slice(pa.array([b"ab"], pa.binary(2)), 0)
    for call in (lambda: sess.ascii_upper(pa.scalar("abc")), lambda: sess.utf8_slice_codeunits(pa.scalar("abc"), 0, 1), lambda: sess.ascii_trim(pa.scalar("abc"), "a")):
        with pytest.raises(ac.ErrNotImplemented, match="takes an array or a chunked array, not a scalar"):
            call()
    with pytest.raises(ac.ArrowError, match="dictionary|no kernel matching"):
        sess.ascii_upper(arr.dictionary_encode())
