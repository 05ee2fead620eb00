"""The OpenEXR output's cases (include/digital_earth_exr.h): the smallest shapes that reach each branch of the file, shared by the CPU tests of the
restatement and the GPU tests, which compare byte for byte.  Each case: name -> (image (H, W, 3) float32 rows top-down, pixel_type, compression,
chunk_bytes, scale).  encoded(name) computes the restatement's file once per process."""
import functools

import numpy as np

import exr_ref

F = np.float32

# the HALF conversion's edges: zeros, the subnormal range and its ties, ties both ways at 1, the clamp, the infinities, NaN (which becomes +0)
HALF_EDGES = np.array([0.0, -0.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -24 * 1.5, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14, 1.0 + 2.0 ** -11, 1.0 + 3.0 * 2.0 ** -11,
                       65504.0, 65519.99, 65520.0, 1e30, np.inf, -np.inf, np.nan,
                       -(2.0 ** -24), -(2.0 ** -25), -(2.0 ** -24 * 1.5), -(2.0 ** -14 - 2.0 ** -24), -(2.0 ** -14), -(1.0 + 2.0 ** -11), -(1.0 + 3.0 * 2.0 ** -11),
                       -65504.0, -65519.99, -65520.0, -1e30, 2.0 ** -25 * (1.0 + 2.0 ** -23), 2.0 ** -15, 2.0 ** -15 * (1.0 + 2.0 ** -10), 0.1, 1.0 / 3.0], F)


def _radiance(H, W, seed):
    """Scene-like sums: a few decades of exposure, flat patches (runs in the predicted bytes) and noise."""
    rng = np.random.default_rng(seed)
    img = (np.exp2(rng.uniform(-9.0, 3.0, (H, W, 1))) * rng.uniform(0.3, 1.6, (H, W, 3))).astype(F)
    flat = np.exp2(np.floor(rng.uniform(-6.0, 2.0, ((H + 7) // 8, (W + 15) // 16, 3)))).astype(F)
    patches = np.repeat(np.repeat(flat, 8, axis=0), 16, axis=1)[:H, :W]
    mask = rng.uniform(size=((H + 7) // 8, (W + 15) // 16)) < 0.6
    mask = np.repeat(np.repeat(mask, 8, axis=0), 16, axis=1)[:H, :W, None]
    return np.where(mask, patches, img).astype(F)


def _random_bits(H, W, seed):
    """Random float32 bit patterns with the NaNs masked out: nothing to compress."""
    bits = np.random.default_rng(seed).integers(0, 1 << 32, (H, W, 3), dtype=np.uint64).astype(np.uint32)
    nan = (bits & 0x7fffffff) > 0x7f800000
    return np.where(nan, bits & np.uint32(0xbfffffff), bits).astype(np.uint32).view(F)


def _half_zero():
    img = np.zeros((64, 48, 3), F)
    img[32:] = _random_bits(32, 48, 11)      # the top two blocks zero (compressed), the bottom two noise (raw)
    return img


def _edges():
    return np.resize(HALF_EDGES, 20 * 13 * 3).reshape(20, 13, 3).astype(F)


CASES = {
    "1x1": (np.array([[[0.25, 1.0, 3.5]]], F), "half", "zip", 16384, 1.0),
    "1x1_none_float": (np.array([[[0.25, 1.0, 3.5]]], F), "float", "none", 16384, 1.0),
    "3x17_zip": (_radiance(17, 3, 1), "half", "zip", 16384, 1.0),      # two blocks, the second of one line
    "700x33_half_1024": (_radiance(33, 700, 2), "half", "zip", 1024, 1.0),      # a block of 67 200 bytes: 66 chunks, segments of more than one byte per thread
    "700x33_float_1024": (_radiance(33, 700, 3), "float", "zip", 1024, 1.0),    # 134 400 bytes: 132 chunks
    "8x1100_zips": (_radiance(1100, 8, 4), "half", "zips", 16384, 1.0),         # 1100 pieces: the scan's run is 2
    "8x1100_none": (_radiance(1100, 8, 4), "half", "none", 16384, 1.0),
    "constant": (np.full((20, 300, 3), (0.5, 0.125, 2.0), F), "half", "zip", 16384, 1.0),      # runs past 258
    "random_bits_float": (_random_bits(20, 40, 5), "float", "zip", 2048, 1.0),        # every block falls back to raw
    "half_zero_float": (_half_zero(), "float", "zip", 4096, 1.0),                       # compressed and raw blocks in one file
    "half_edges": (_edges(), "half", "zip", 16384, 1.0),
    "half_edges_float": (_edges(), "float", "zips", 16384, 1.0),
    "scale_half": (_radiance(5, 7, 6), "half", "zip", 16384, 0.5),
    "scale_3": (_radiance(5, 7, 6), "float", "zips", 16384, 3.0),
}


@functools.lru_cache(maxsize=None)
def encoded(name):
    image, pixel_type, compression, chunk, scale = CASES[name]
    info = []
    return exr_ref.encode(image, pixel_type, compression, chunk, scale, info=info), tuple(info)
