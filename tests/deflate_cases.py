"""Inputs that reach the branches of the shared deflate coder (csrc/png_deflate.h: png_code_chunk, png_code_lengths) which the cases of
tests/png_cases.py and tests/exr_cases.py leave cold: the 15-bit length limit, chunks of the full 65 535 bytes, every one of the 29 length codes, and
chunk lengths around the 512-thread split.  Pure numpy, seeded; shared by the CPU tests, which prove that each input reaches what it is here for
(tests/test_deflate_cases.py), and the GPU tests, which compare byte for byte (tests/test_gpu_deflate_edges.py).
PNG_CASES: name -> (pixels, filter, chunk_bytes), as png_cases.CASES; EXR_CASES: name -> (image, pixel_type, compression, chunk_bytes, scale), as
exr_cases.CASES.  png_encoded(name) / exr_encoded(name) compute the restatement's file once per process."""
import functools

import numpy as np

import exr_cases
import exr_ref
import png_ref

F = np.float32
FULL = 65535      # the largest chunk the settings take


def chain_counts(nsym):
    """Counts whose Huffman tree, with end-of-block's one occurrence among them, is a chain: each exceeds everything merged two steps before it."""
    counts, s_prev, s = [1], 1, 2      # s: the sum so far, end-of-block counted in
    while len(counts) < nsym:
        c = s_prev + 1
        counts.append(c)
        s_prev, s = s, s + c
    return counts


def chain_bytes(nsym, multiple, seed, lead=None):
    """Bytes whose literal histogram forces a chain-shaped Huffman tree over nsym literals and end-of-block: depth nsym unlimited.  The most frequent
    symbol's count grows until the length is a multiple of `multiple`.  Values: the first of default_rng(seed).permutation(256); laid out
    most-frequent-first into the even positions, then the odd ones, so that no two neighbours are equal and every token is a literal.
    lead=None: all nsym symbols are free and returned.  lead=v: the rarest symbol is the single byte v that the caller puts in front (a PNG row's filter
    byte); the nsym - 1 others, with values != v, are returned."""
    counts = chain_counts(nsym)
    perm = [int(v) for v in np.random.default_rng(seed).permutation(256)]
    if lead is not None:
        counts = counts[1:]
        perm = [v for v in perm if v != lead]
    values = perm[:len(counts)]
    while sum(counts) % multiple:
        counts[-1] += 1
    total = sum(counts)
    assert 2 * counts[-1] <= total + (0 if lead is None else 1)      # at most half of everything coded
    seq = np.repeat(np.array(values[::-1], np.uint8), counts[::-1])
    half = (total + 1) // 2
    out = np.empty(total, np.uint8)
    out[0::2] = seq[:half]
    out[1::2] = seq[half:]
    assert (out[1:] != out[:-1]).all() and (lead is None or out[0] != lead)
    return out.tobytes()


def unpredict(p):
    """The inverse of exr_ref.predict: the running sum of p - 128 from p[0], then the two halves interleaved again."""
    p = np.frombuffer(bytes(p), np.uint8).astype(np.int64)
    t = p.copy()
    t[1:] = p[1:] - 128
    t = (np.cumsum(t) & 255).astype(np.uint8)
    half = (len(t) + 1) // 2
    r = np.empty(len(t), np.uint8)
    r[0::2] = t[:half]
    r[1::2] = t[half:]
    assert np.array_equal(exr_ref.predict(r.tobytes()), p.astype(np.uint8))
    return r.tobytes()


def _row(data):
    """Bytes (a multiple of 3) as a one-row RGB8 image."""
    return np.frombuffer(bytes(data), np.uint8).reshape(1, -1, 3).copy()


def _chain_row(nsym, seed):
    return _row(chain_bytes(nsym, 3, seed, lead=0))      # filter "none": the row's type byte 0 is the rarest symbol


def _noise(shape, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, shape).astype(np.uint8)


def _noise_on_gradient(H, W, seed):
    """png_cases._noise_on_gradient at another size."""
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([(x * 255) // (W - 1), (y * 255) // (H - 1), ((x + y) * 255) // (H + W - 2)], axis=-1)
    return np.clip(base + np.random.default_rng(seed).integers(-3, 4, base.shape), 0, 255).astype(np.uint8)


def length_code_runs():
    """The runs r (equal bytes behind a run's head) of the all_length_codes row: the bottom and the top of every length code's range, and the runs
    around and past 258 that the remainder rule splits."""
    base, top = png_ref.LEN_BASE, png_ref.LEN_BASE + (1 << png_ref.LEN_EXTRA) - 1
    return sorted(set(int(v) for v in base) | set(int(v) for v in top) | {259, 260, 261, 262, 517, 775})


def _all_length_codes(seed):
    rng = np.random.default_rng(seed)
    out, prev = [], 0      # the filter byte in front of the row
    for r in length_code_runs():
        v = int(rng.choice([x for x in range(1, 256) if x != prev]))
        sep = int(rng.choice([x for x in range(1, 256) if x != v]))
        out += [v] * (r + 1) + [sep]
        prev = sep
    out += [prev] * (-len(out) % 3)
    return _row(out)


def _split_row(W, seed):
    """test_tokens_expand_back_to_the_chunk's generator, cut to a row of W pixels."""
    rng = np.random.default_rng(seed)
    return _row(np.repeat(rng.integers(0, 256, 40), rng.integers(1, 700, 40)).astype(np.uint8)[:3 * W])


def exr_chain_image(seed):
    """chain_bytes(16, 12, seed) as the predicted bytes of a one-line FLOAT block: unpredicted, read as little-endian floats, the planes B, G, R."""
    r = np.frombuffer(unpredict(chain_bytes(16, 12, seed)), "<f4")
    W = len(r) // 3
    return np.ascontiguousarray(np.stack([r[2 * W:], r[W:2 * W], r[:W]], axis=-1)[None].astype(F))


@functools.lru_cache(maxsize=None)
def exr_chain_seed():
    """The first seed whose floats are all finite and zero or normal: a NaN would be stored as +0, and the bytes would no longer be the chain."""
    for seed in range(4096):
        bits = exr_chain_image(seed).view(np.uint32) & 0x7fffffff
        if ((bits == 0) | ((bits >= 0x00800000) & (bits < 0x7f800000))).all():
            return seed
    raise AssertionError("no seed below 4096 gives finite, normal floats")


CHAIN16 = _chain_row(16, 16)

PNG_CASES = {
    "chain16": (CHAIN16, "none", 4180),
    "chain17": (_chain_row(17, 17), "none", 6763),
    "chain21": (_chain_row(21, 21), "none", 46366),
    "chain16_first_of_two": (np.concatenate((CHAIN16, _noise((1, CHAIN16.shape[1], 3), 0, 255, 22))), "none", 4180),
    "noise_65535": (_noise((150, 148, 3), 0, 255, 23), "none", FULL),
    "white_65535": (np.full((150, 148, 3), 255, np.uint8), "none", FULL),
    "black_65535": (np.zeros((150, 148, 3), np.uint8), "none", FULL),      # type byte 0 and pixels 0: the whole first chunk is one run
    "high_65535": (_noise((150, 148, 3), 250, 255, 24), "none", FULL),
    "default_chunk": (_noise_on_gradient(150, 148, 25), "adaptive", png_ref.DEFAULT_CHUNK),
    "all_length_codes": (_all_length_codes(26), "none", 16384),
}
for _W in (170, 171, 341, 342):
    PNG_CASES["split_%d" % (1 + 3 * _W)] = (_split_row(_W, 27 + _W), "none", 2048)

EXR_CASES = {
    "exr_chain16": (exr_chain_image(exr_chain_seed()), "float", "zips", 4188, 1.0),
    "exr_noise_65535": (exr_cases._random_bits(16, 342, 28), "float", "zip", FULL, 1.0),
    "exr_const_65535": (np.full((16, 342, 3), (0.5, 0.125, 2.0), F), "float", "zip", FULL, 1.0),
}


@functools.lru_cache(maxsize=None)
def png_encoded(name):
    px, flt, chunk = PNG_CASES[name]
    info = []
    return png_ref.encode(px, flt, chunk, info=info), tuple(info)


@functools.lru_cache(maxsize=None)
def exr_encoded(name):
    image, pixel_type, compression, chunk, scale = EXR_CASES[name]
    info = []
    return exr_ref.encode(image, pixel_type, compression, chunk, scale, info=info), tuple(info)
