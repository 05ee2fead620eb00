"""The PNG output's cases (include/digital_earth_png.h): the smallest shapes that reach each branch of the stream, shared by the CPU tests of the
restatement and the GPU tests, which compare byte for byte.  Each case: name -> (pixels, filter, chunk_bytes); pixels are (H, W, C) uint8 or
(H, W, 3) uint16, rows top-down.  encoded(name) computes the restatement's file once per process."""
import functools

import numpy as np

import png_ref


def _noise(shape, dtype, seed):
    info = np.iinfo(dtype)
    return np.random.default_rng(seed).integers(0, info.max + 1, shape).astype(dtype)


def _half_black():
    px = np.zeros((64, 64, 3), np.uint8)
    px[32:] = _noise((32, 64, 3), np.uint8, 5)      # the upper half black (runs cut at chunk edges), the lower noise (stored blocks)
    return px


def _noise_on_gradient():
    y, x = np.mgrid[0:600, 0:600]
    base = np.stack([(x * 255) // 599, (y * 255) // 599, ((x + y) * 255) // 1198], axis=-1)
    return np.clip(base + np.random.default_rng(6).integers(-3, 4, base.shape), 0, 255).astype(np.uint8)


def _smooth16():
    y, x = np.mgrid[0:17, 0:33]
    return np.stack([x * 1985 + y * 3, y * 3855 + 255, (x * y) * 124], axis=-1).astype(np.uint16)


CASES = {
    "1x1_rgb8": (np.array([[[17, 0, 255]]], np.uint8), "adaptive", 16384),
    "7x5_rgb8": (_noise((5, 7, 3), np.uint8, 1), "adaptive", 16384),
    "7x5_rgba8": (_noise((5, 7, 4), np.uint8, 2), "adaptive", 16384),
    "33x17_rgb16": (_smooth16(), "adaptive", 16384),
    "33x17_rgb16_noise": (_noise((17, 33, 3), np.uint16, 3), "adaptive", 1024),
    "300x3_constant_rgba": (np.full((3, 300, 4), (200, 100, 50, 255), np.uint8), "adaptive", 16384),
    "64x64_half_black": (_half_black(), "adaptive", 1024),
    "600x600_noise_on_gradient": (_noise_on_gradient(), "adaptive", 1024),      # 1056 chunks: more than one trip of the 1024-thread scan
}
for _f in ("none", "sub", "up", "average", "paeth"):
    CASES["16x9_%s" % _f] = ((_noise((9, 16, 3), np.uint8, 4) >> 5 << 5), _f, 16384)


@functools.lru_cache(maxsize=None)
def encoded(name):
    px, flt, chunk = CASES[name]
    info = []
    return png_ref.encode(px, flt, chunk, info=info), tuple(info)
