"""CPU tests of the deflate coder's edge cases (tests/deflate_cases.py): each input reaches the branch it is there for — measured on the restatement
(tests/png_ref.py, tests/exr_ref.py), so that the GPU's byte-for-byte test (tests/test_gpu_deflate_edges.py) cannot pass without running it — and
every restatement file decodes to its input through zlib.  The unlimited depth is that of a heap-built Huffman tree; the chain histograms leave it no
choice, and the limit binds wherever it exceeds 15."""
import heapq
import struct

import numpy as np
import pytest

import deflate_cases as dc
import exr_cases
import exr_ref
import png_cases
import png_ref
from digital_earth_amd import exr


def _unlimited_depth(freq):
    """The longest code of a Huffman tree built with a heap, as in test_code_lengths_are_huffman_where_no_limit_binds."""
    heap = [(f, i, (i,)) for i, f in enumerate(freq) if f]
    depth = dict.fromkeys((i for i, f in enumerate(freq) if f), 0)
    heapq.heapify(heap)
    tick = len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            depth[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2])); tick += 1
    return max(depth.values())


@pytest.fixture
def trees(monkeypatch):
    """png_ref.code_lengths wrapped: per chunk coded while the test runs, (unlimited depth, longest length handed out, Kraft sum in units of 2^-15)."""
    seen, inner = [], png_ref.code_lengths

    def recording(freq):
        ll = inner(freq)
        seen.append((_unlimited_depth([int(f) for f in freq]), max(ll), sum(1 << (15 - l) for l in ll if l)))
        return ll
    monkeypatch.setattr(png_ref, "code_lengths", recording)
    return seen


def _png(name, trees):
    px, flt, chunk = dc.PNG_CASES[name]
    cached = dc.png_encoded(name)
    del trees[:]
    info = []
    data = png_ref.encode(px, flt, chunk, info=info)      # (not the cached file alone: the wrapper has to see exactly this case's chunks)
    assert data == cached[0] and tuple(info) == cached[1]
    return data, info


def _length_codes(name):
    px, flt, chunk = dc.PNG_CASES[name]
    S = png_ref.filtered_stream(px, flt)
    assert len(S) <= chunk
    L = png_ref.tokens(S)[1]
    return L[L > 0], set(int(c) for c in png_ref.LEN_CODE[L[L > 0] - 3])


# ---------------------------------------------------------------- the generators
@pytest.mark.parametrize("nsym,multiple,lead", [(16, 3, 0), (17, 3, 0), (21, 3, 0), (16, 12, None), (3, 1, None), (9, 7, 5)])
def test_chain_bytes_are_all_literals_on_a_chain(nsym, multiple, lead):
    b = np.frombuffer(dc.chain_bytes(nsym, multiple, 3, lead=lead), np.uint8)
    assert len(b) % multiple == 0 and (b[1:] != b[:-1]).all()
    counts = np.bincount(b, minlength=256)
    if lead is not None:
        assert counts[lead] == 0
        counts[lead] = 1
    want = dc.chain_counts(nsym)
    got = sorted(int(c) for c in counts if c)
    assert got[:-1] == want[:-1] and 0 <= got[-1] - want[-1] < multiple and 2 * got[-1] <= sum(got)
    freq = [int(c) for c in counts] + [1]      # end-of-block
    assert _unlimited_depth(freq) == nsym


def test_unpredict_inverts_the_predictor():
    rng = np.random.default_rng(31)
    for n in (1, 2, 3, 8, 4187, 4188):
        p = rng.integers(0, 256, n).astype(np.uint8)
        r = dc.unpredict(p.tobytes())
        assert len(r) == n and np.array_equal(exr_ref.predict(r), p)
    r = rng.integers(0, 256, 1001).astype(np.uint8).tobytes()
    assert dc.unpredict(exr_ref.predict(r).tobytes()) == r


def test_exr_chain_image_is_the_first_finite_normal_seed_and_keeps_its_bytes():
    assert dc.exr_chain_seed() == 37
    image = dc.EXR_CASES["exr_chain16"][0]
    assert image.shape == (1, 349, 3) and np.isfinite(image).all()
    r = exr_ref.raw_block(exr_ref.convert(image, 1.0, "float"))
    assert exr_ref.predict(r).tobytes() == dc.chain_bytes(16, 12, 37)      # what the coder sees is the chain


# ---------------------------------------------------------------- what each case reaches
@pytest.mark.parametrize("name,N,depths,blocks", [
    ("chain16", 4180, [16], ["dynamic"]),
    ("chain17", 6763, [17], ["dynamic"]),
    ("chain21", 46366, [21], ["dynamic"]),
    ("chain16_first_of_two", 8360, [16, None], ["dynamic", "stored"]),
])
def test_chain_cases_reach_the_length_limit(trees, name, N, depths, blocks):
    data, info = _png(name, trees)
    px, flt, chunk = dc.PNG_CASES[name]
    assert len(png_ref.filtered_stream(px, flt)) == N and info == blocks and len(trees) == len(depths)
    for (unlimited, longest, kraft), want in zip(trees, depths):
        print("%s: unlimited depth %d, longest code %d, Kraft sum %d / 32768" % (name, unlimited, longest, kraft))
        assert kraft == 1 << 15
        if want is not None:
            assert unlimited == want and longest == 15
        else:
            assert unlimited <= 15 and longest == unlimited
    assert np.array_equal(png_ref.decode(data)[0], px)


def test_chain21_gives_a_thread_91_bytes():
    assert -(-46366 // 512) == 91


def test_exr_chain_reaches_the_limit_and_stays_compressed(trees):
    image, pixel_type, compression, chunk, scale = dc.EXR_CASES["exr_chain16"]
    cached = dc.exr_encoded("exr_chain16")[0]
    del trees[:]
    info = []
    data = exr_ref.encode(image, pixel_type, compression, chunk, scale, info=info)
    print("exr_chain16: unlimited depth %d, longest code %d, Kraft sum %d / 32768" % trees[0])
    assert trees == [(16, 15, 1 << 15)] and info == ["zip"] and data == cached


@pytest.mark.parametrize("name,blocks,size", [
    ("noise_65535", ["stored", "stored"], 66852),
    ("white_65535", ["dynamic", "dynamic"], 700),
    ("black_65535", ["dynamic", "dynamic"], None),
    ("high_65535", ["dynamic", "dynamic"], None),
    ("default_chunk", ["dynamic", "dynamic", "dynamic"], None),
])
def test_full_chunks(trees, name, blocks, size):
    data, info = _png(name, trees)
    px, flt, chunk = dc.PNG_CASES[name]
    S = png_ref.filtered_stream(px, flt)
    assert len(S) == 66750 and info == blocks and all(k == 1 << 15 for _, _, k in trees)
    assert [min(chunk, len(S) - lo) for lo in range(0, len(S), chunk)] == ([65535, 1215] if chunk == dc.FULL else [32768, 32768, 1214])
    assert size is None or len(data) == size
    assert np.array_equal(png_ref.decode(data)[0], px)
    assert len(data) <= png_ref.capacity(148, 150, 3, 8, chunk)


def test_noise_65535_first_stored_block_has_len_ffff():
    data = dc.png_encoded("noise_65535")[0]
    at = 33                                                        # behind the signature and IHDR: the first IDAT
    n, kind = struct.unpack(">I4s", data[at:at + 8])
    assert kind == b"IDAT" and n == 2 + 5 + 65535 + 5
    body = data[at + 8:at + 8 + n]
    assert body[:3] == b"\x78\x01\x00" and struct.unpack("<HH", body[3:7]) == (0xffff, 0x0000)
    assert body[-5:] == b"\x00\x00\x00\xff\xff"                    # the empty stored block behind a non-final chunk


def test_black_65535_is_one_run_through_the_whole_chunk():
    """Type byte 0 and black pixels: 65 535 equal bytes — the literal, 254 matches of 258, and the remainder 2 as literals."""
    px, flt, chunk = dc.PNG_CASES["black_65535"]
    v, L = png_ref.tokens(png_ref.filtered_stream(px, flt)[:chunk])
    assert list(L) == [0] + [258] * 254 + [0, 0] and set(v) == {0}


def test_white_65535_runs_end_at_every_row():
    """Type byte 0 in front of 444 bytes of 255: per row two literals, a match of 258 and one of 185."""
    px, flt, chunk = dc.PNG_CASES["white_65535"]
    v, L = png_ref.tokens(png_ref.filtered_stream(px, flt)[:445 * 3])
    assert list(L) == [0, 0, 258, 185] * 3


def test_high_65535_has_the_largest_adler_partials_of_a_dynamic_block():
    px, flt, chunk = dc.PNG_CASES["high_65535"]
    S = png_ref.filtered_stream(px, flt)[:chunk].astype(np.int64)
    B = int(((len(S) - np.arange(len(S))) * S).sum())
    assert S.mean() > 250 and B > 250 * 65535 * 65536 // 2         # 5.4e11: far past 32 bits before the % 65521


def test_all_length_codes_emits_all_29_and_the_ends_of_every_range():
    lengths, codes = _length_codes("all_length_codes")
    print("all_length_codes: %d of 29 length codes, %d filtered bytes, a thread's segment %d bytes"
          % (len(codes), 1 + dc.PNG_CASES["all_length_codes"][0].size, -(-(1 + dc.PNG_CASES["all_length_codes"][0].size) // 512)))
    assert len(codes) == 29
    top = png_ref.LEN_BASE + (1 << png_ref.LEN_EXTRA) - 1
    assert set(int(v) for v in png_ref.LEN_BASE) | set(int(v) for v in top) <= set(int(v) for v in lengths)
    assert 9 in lengths                                            # code 263, which no older case emits
    runs = dc.length_code_runs()
    assert {259, 260, 261, 262, 517, 775} <= set(runs) and (np.diff(np.flatnonzero(lengths == 258)) == 1).any()      # 517, 775: 258 twice in a row
    assert -(-(1 + dc.PNG_CASES["all_length_codes"][0].size) // 512) <= min(runs[8:])     # 1 + r bytes: the longer runs all cross thread segments


def test_all_length_codes_decodes(trees):
    data, info = _png("all_length_codes", trees)
    assert info == ["dynamic"] and np.array_equal(png_ref.decode(data)[0], dc.PNG_CASES["all_length_codes"][0])


@pytest.mark.parametrize("N,threads,seg", [(511, 511, 1), (514, 257, 2), (1024, 512, 2), (1027, 343, 3)])
def test_split_cases_sit_around_the_thread_split(trees, N, threads, seg):
    name = "split_%d" % N
    data, info = _png(name, trees)
    px, flt, chunk = dc.PNG_CASES[name]
    S = png_ref.filtered_stream(px, flt)
    assert len(S) == N and chunk >= N and info == ["dynamic"]
    assert -(-N // 512) == seg and -(-N // seg) == threads         # the segment, and the threads that own a byte
    assert (N % seg != 0) == (N == 1027)                           # only 1027 leaves its last thread a ragged segment
    starts = np.flatnonzero(np.concatenate(([True], S[1:] != S[:-1])))
    assert (np.diff(np.concatenate((starts, [N]))) > 2 * seg).any()      # a run that passes through a whole segment
    assert np.array_equal(png_ref.decode(data)[0], px)


@pytest.mark.parametrize("name,blocks,pieces", [("exr_noise_65535", ["raw"], [65535, 129]), ("exr_const_65535", ["zip"], [65535, 129])])
def test_exr_full_pieces(trees, name, blocks, pieces):
    image, pixel_type, compression, chunk, scale = dc.EXR_CASES[name]
    cached = dc.exr_encoded(name)[0]
    del trees[:]
    info = []
    data = exr_ref.encode(image, pixel_type, compression, chunk, scale, info=info)
    P = image.size * 4
    assert P == 65664 and [min(chunk, P - lo) for lo in range(0, P, chunk)] == pieces and len(trees) == 2
    assert info == blocks and data == cached
    if blocks == ["zip"]:
        block_info = []
        exr_ref.zip_payload(exr_ref.raw_block(exr_ref.convert(image, scale, pixel_type)), chunk, block_info)
        assert block_info[0] == "dynamic"                          # the full piece is coded, not stored


@pytest.mark.parametrize("name", sorted(dc.EXR_CASES))
def test_exr_restatement_reads_back(name):
    image, pixel_type, compression, chunk, scale = dc.EXR_CASES[name]
    data, blocks = dc.exr_encoded(name)
    back, info = exr.read(data)
    want = exr_ref.convert(image, scale, pixel_type)
    assert np.array_equal(back.view(np.uint32), want.view(np.uint32))
    assert [("raw" if b["raw"] else "zip") for b in info["blocks"]] == list(blocks)
    assert len(data) <= exr_ref.capacity(image.shape[1], image.shape[0], pixel_type, compression)


# ---------------------------------------------------------------- why these cases exist
def test_older_cases_never_reach_the_length_limit(trees):
    """Over every chunk of png_cases.CASES and exr_cases.CASES the unlimited tree stays within 15 bits: the repair in png_code_lengths runs on none of
    them.  (Should this fail one day, the older cases have begun to cover the limit too, which is harmless: raise the bound or drop this test.)"""
    for name, (px, flt, chunk) in sorted(png_cases.CASES.items()):
        png_ref.encode(px, flt, chunk)
    for name, (image, pixel_type, compression, chunk, scale) in sorted(exr_cases.CASES.items()):
        exr_ref.encode(image, pixel_type, compression, chunk, scale)
    deepest = max(d for d, _, _ in trees)
    print("older cases: %d chunks, deepest unlimited tree %d" % (len(trees), deepest))
    assert len(trees) > 2000 and deepest <= 15 and all(k == 1 << 15 for _, _, k in trees)
