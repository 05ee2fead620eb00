"""The case list of the Radiance HDR output's tests (CPU: tests/test_rgbe_ref.py; GPU: tests/test_gpu_rgbe.py; the widths also in
tools/rgbe_host_check.cpp): name -> (image (H, W, 3) float32 rows top-down, rle, rounding, scale).  The widths stand around what the coder treats
differently: below the format's 8, the packets' 127 and 128, two packets (254, 255, 257), a span of two bytes per thread (257, 300), 4400 pieces
(8 x 1100: more than one piece per thread of the scan), the widest coded row and the first flat one."""
import functools

import numpy as np

import rgbe_ref as gr

F = np.float32
WIDTHS = (1, 7, 8, 9, 127, 128, 129, 254, 255, 257, 300)


def _stretches(W, lengths, rng):
    """A row of W pixels in stretches of the given lengths in turn, each of one colour that differs from its neighbour's in every plane."""
    row, x, k = np.zeros((W, 3), F), 0, 0
    palette = np.array([[0.9, 0.3, 0.1], [0.02, 0.6, 0.4], [7.0, 1.5, 0.2], [0.3, 0.01, 110.0]], F)
    while x < W:
        n = lengths[k % len(lengths)]
        row[x:x + n] = palette[k % 4] * F(1 + (k // 4) % 3)
        x, k = x + n, k + 1
    return row


def _noise(W, rng):
    return np.exp(rng.uniform(-9.0, 9.0, (W, 3))).astype(F)


def _ramp(W):
    x = (np.arange(W) // 5).astype(F) / F(max(W // 5, 1))           # plateaus of five pixels: runs in some planes, literals in others
    return np.stack([x * F(4), x * x, F(1) - x * F(0.5)], axis=-1).astype(F)


def _rows(W, H, seed):
    rng = np.random.default_rng(seed)
    kinds = (lambda: np.tile(np.array([[0.5, 0.25, 0.125]], F), (W, 1)), lambda: _stretches(W, (3, 4), rng), lambda: _stretches(W, (127, 128, 254), rng),
             lambda: _noise(W, rng), lambda: _ramp(W))
    if H == 1:                                                      # one row of everything: stretches of 3 and 4, noise, a long constant stretch
        row = _stretches(W, (3, 4, 4, 3, 1, 2), rng)
        row[W // 3:2 * W // 3] = _noise(W, rng)[W // 3:2 * W // 3]
        row[2 * W // 3:] = row[-1]
        return row[None]
    return np.stack([kinds[y % 5]() for y in range(H)])


def _special():
    v = np.array([np.nan, np.inf, -np.inf, -1.0, 1e-33, 1e-45, 2.0 ** 127, 255 * 2.0 ** 119, 0.9999999, 1.0, 0.18, 65504.0, 1e-32, 0.99e-32, -0.0, 0.0], F)
    img = np.zeros((3, 16, 3), F)
    img[0, :, 0] = v                                                # each alone
    img[1, :, 1] = v; img[1, :, 0] = F(1.0)                         # beside 1
    img[2, :, 2] = v; img[2, :, 1] = np.roll(v, 5); img[2, :, 0] = np.roll(v, 11)
    return img


def _make():
    cases = {}
    for i, W in enumerate(WIDTHS):
        for H in (1, 5):
            cases["w%03d_h%d" % (W, H)] = (_rows(W, H, 100 * i + H), True, "trunc", 1.0)
    tall = np.repeat(_rows(8, 5, 7), 220, axis=0)                   # 8 x 1100: 4400 pieces
    tall[::7] = _noise(8, np.random.default_rng(8))
    cases["tall_8x1100"] = (tall, True, "trunc", 1.0)
    cases["widest_rle_32767"] = (_rows(32767, 1, 9), True, "trunc", 1.0)
    cases["first_flat_32768"] = (_rows(32768, 1, 10), True, "trunc", 1.0)
    cases["special"] = (_special(), True, "trunc", 1.0)
    cases["special_round"] = (_special(), True, "round", 1.0)
    cases["w129_h5_round"] = (_rows(129, 5, 11), True, "round", 1.0)
    cases["w300_h5_flat"] = (_rows(300, 5, 12), False, "trunc", 1.0)
    cases["w257_h5_scale"] = (_rows(257, 5, 13), True, "round", 0.25)
    return cases


CASES = _make()
# (R, G, B), rounding -> the four bytes: checked on the CPU when the format was stated
KNOWN = (((1, 1, 1), "trunc", "80808081"), ((0.5, 0.25, 0.125), "trunc", "80402080"), ((0.18, 0.18, 0.18), "trunc", "B8B8B87E"),
         ((65504, 1, 0), "trunc", "FF000090"), ((255 * 2.0 ** 119, 0, 0), "trunc", "FF0000FF"), ((0.9999999, 0, 0), "trunc", "FF000080"),
         ((0.9999999, 0, 0), "round", "80000081"))


@functools.lru_cache(maxsize=None)
def encoded(name):
    image, rle, rounding, scale = CASES[name]
    return gr.encode(image, rle, rounding, scale)
