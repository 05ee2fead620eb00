"""CPU tests of the PNG output's restatement (tests/png_ref.py; include/digital_earth_png.h is the contract): it decodes to its input through an
independent inflater, the filter equals a naive loop, the tokens follow the run rule, the code lengths stay complete within 15 bits, and the stored
fallback triggers exactly where it should."""
import heapq
import zlib

import numpy as np
import pytest

import png_cases
import png_ref


@pytest.mark.parametrize("name", sorted(png_cases.CASES))
def test_restatement_decodes_to_its_input(name):
    px = png_cases.CASES[name][0]
    data, _ = png_cases.encoded(name)
    got, info = png_ref.decode(data)
    assert got.dtype == px.dtype and np.array_equal(got, px)
    assert (info["cicp"] == bytes((1, 8, 0, 1))) if px.dtype == np.uint16 else (info["cicp"] is None)
    N = px.shape[0] * (1 + px.shape[1] * px.shape[2] * px.dtype.itemsize)
    assert info["idats"] == -(-N // png_cases.CASES[name][2]) + 1
    assert len(data) <= png_ref.capacity(px.shape[1], px.shape[0], px.shape[2], 8 * px.dtype.itemsize, png_cases.CASES[name][2])


@pytest.mark.parametrize("name", ["7x5_rgb8", "7x5_rgba8", "33x17_rgb16", "33x17_rgb16_noise", "300x3_constant_rgba", "16x9_none"])
def test_adaptive_filter_equals_a_naive_loop(name):
    rows, bpp, _, _ = png_ref.as_rows(png_cases.CASES[name][0])
    S, types = png_ref.filter_rows(rows, bpp, "adaptive")
    assert np.array_equal(S, png_ref.filter_rows_naive(rows, bpp))
    assert np.array_equal(S[:, 0], types)


def test_constant_rows_differ_in_their_filter_bytes():
    """300 x 3 constant RGBA: the first row cannot use Up, the others can: the runs cross row ends at differing type bytes."""
    rows, bpp, _, _ = png_ref.as_rows(png_cases.CASES["300x3_constant_rgba"][0])
    types = png_ref.filter_rows(rows, bpp)[1]
    assert types[0] != types[1] and types[1] == types[2] == 2


def test_tokens_expand_back_to_the_chunk():
    rng = np.random.default_rng(11)
    chunks = [rng.integers(0, 256, 1000).astype(np.uint8), rng.integers(0, 2, 3000).astype(np.uint8), np.zeros(5000, np.uint8),
              np.repeat(rng.integers(0, 256, 40), rng.integers(1, 700, 40)).astype(np.uint8), np.array([7], np.uint8)]
    for c in chunks:
        v, L = png_ref.tokens(c)
        assert png_ref.expand(v, L) == c.tobytes()
        assert ((L == 0) | ((L >= 3) & (L <= 258))).all()


@pytest.mark.parametrize("run,expect", [(1, [0]), (2, [0, 0]), (3, [0, 0, 0]), (4, [0, 3]), (259, [0, 258]), (260, [0, 258, 0]), (261, [0, 258, 0, 0]),
                                        (262, [0, 258, 3]), (517, [0, 258, 258])])
def test_tokens_follow_the_258_and_remainder_rule(run, expect):
    """`run` equal bytes between two others: the literal, r / 258 matches of 258, then one match of r mod 258 if that is >= 3, else literals."""
    c = np.array([1] + [9] * run + [2], np.uint8)
    v, L = png_ref.tokens(c)
    assert list(L) == [0] + expect + [0] and set(v[1:-1]) == {9}
    assert png_ref.expand(v, L) == c.tobytes()


def _kraft(lengths):
    return sum(2.0 ** -l for l in lengths if l)


def test_code_lengths_complete_and_limited_on_skewed_histograms():
    fib = [1, 1]
    while len(fib) < 40:
        fib.append(fib[-1] + fib[-2])       # unlimited Huffman lengths would reach 39 bits
    for freq in (fib, fib[:20] + [0] * 10 + fib[20:30], [1] * 286, [1, 1], [5, 0, 0, 1], [1] * 285 + [10 ** 6], list(range(1, 287))):
        ll = png_ref.code_lengths(freq)
        assert max(ll) <= 15 and all((l > 0) == (f > 0) for l, f in zip(ll, freq))
        assert _kraft(ll) == 1.0
        codes = png_ref.canonical_codes(ll)
        assert len({(l, c) for l, c in zip(ll, codes) if l}) == sum(1 for l in ll if l)


def test_code_lengths_are_huffman_where_no_limit_binds():
    """Against a heap-built Huffman tree: the same total cost whenever the longest code stays within 15 bits."""
    rng = np.random.default_rng(12)
    for _ in range(20):
        freq = [int(f) for f in rng.integers(0, 200, 286)]
        freq[256] = 1
        heap = [(f, i, (i,)) for i, f in enumerate(freq) if f]
        depth = dict.fromkeys((i for i, f in enumerate(freq) if f), 0)
        heapq.heapify(heap)
        tick = len(freq)
        while len(heap) > 1:
            a, b = heapq.heappop(heap), heapq.heappop(heap)
            for s in a[2] + b[2]:
                depth[s] += 1
            heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2])); tick += 1
        ll = png_ref.code_lengths(freq)
        if max(depth.values()) <= 15:
            assert sum(f * l for f, l in zip(freq, ll)) == sum(freq[s] * d for s, d in depth.items())


def test_stored_fallback_on_uniform_noise():
    px = np.random.default_rng(13).integers(0, 256, (40, 40, 3)).astype(np.uint8)
    info = []
    data = png_ref.encode(px, "none", 1024, info=info)
    assert set(info) == {"stored"}
    assert np.array_equal(png_ref.decode(data)[0], px)


@pytest.mark.parametrize("chunk", [1024, 16384])
def test_black_image_is_dynamic_and_small(chunk):
    px = np.zeros((120, 160, 3), np.uint8)
    info = []
    data = png_ref.encode(px, "adaptive", chunk, info=info)
    assert set(info) == {"dynamic"}
    assert len(data) <= 33 + 256 * len(info) + png_ref.TRAILER_BYTES
    assert np.array_equal(png_ref.decode(data)[0], px)


def test_half_black_case_holds_both_block_types():
    info = png_cases.encoded("64x64_half_black")[1]
    assert "stored" in info and "dynamic" in info


def test_large_case_has_more_chunks_than_one_scan_trip():
    assert len(png_cases.encoded("600x600_noise_on_gradient")[1]) == 1056


def test_adler_and_filtered_stream():
    px = png_cases.CASES["7x5_rgb8"][0]
    S = png_ref.filtered_stream(px)
    data = png_cases.encoded("7x5_rgb8")[0]
    assert data[-28:-20] == b"\x00\x00\x00\x04IDAT"
    assert int.from_bytes(data[-20:-16], "big") == zlib.adler32(S.tobytes())
