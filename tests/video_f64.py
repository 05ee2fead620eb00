"""The video frame output stated once more, in float64 and straight from the equations of ITU-T H.273 (and the chroma sample positions of H.264
Annex E / BT.2020): no code shared with tests/video_ref.py, loops over samples instead of strided slices, exact coefficients.

    values(image, bits, matrix, full_range, siting)  ->  (y, cb, cr) float64 planes of code values BEFORE quantisation and clipping to integers,
                                                          clipped to the legal range; rows top-down

H.273:  E'Y = Kr E'R + (1 - Kr - Kb) E'G + Kb E'B,   E'PB = 0.5 (E'B - E'Y) / (1 - Kb),   E'PR = 0.5 (E'R - E'Y) / (1 - Kr)
        limited:  Y = (219 E'Y + 16) 2^(n-8),  Cb = (224 E'PB + 128) 2^(n-8);      full:  Y = (2^n - 1) E'Y,  Cb = (2^n - 1) E'PB + 2^(n-1)
Chroma sample (i, j) sits at luma position (2i + 0.5, 2j + 0.5) for "center", (2i, 2j + 0.5) for "left", (2i, 2j) for "topleft"; a position between two
luma samples takes their mean, a position on one takes [1 2 1] / 4 around it (the shortest symmetric low-pass), edges repeated."""
import math

import numpy as np

K = {"bt709": (0.2126, 0.0722), "bt601": (0.299, 0.114), "bt2020": (0.2627, 0.0593)}


def _unit(t):
    if not (t > 0.0):          # NaN, -0.0 and everything negative
        return 0.0
    return 1.0 if t >= 1.0 else float(t)


def _taps(position2, n):
    """[(index, weight)] for the position `position2` / 2 on an axis of n samples."""
    if position2 % 2:                                     # half-way between (position2 - 1) / 2 and the next
        a = (position2 - 1) // 2
        return [(a, 0.5), (a + 1, 0.5)]
    a = position2 // 2
    return [(min(max(a - 1, 0), n - 1), 0.25), (a, 0.5), (min(a + 1, n - 1), 0.25)]


def values(image, bits=8, matrix="bt709", full_range=False, siting="left"):
    image = np.asarray(image)
    W, H = image.shape[:2]
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    ey = np.zeros((H, W)); pb = np.zeros((H, W)); pr = np.zeros((H, W))
    for x in range(W):
        for r in range(H):
            R, G, B = (_unit(float(t)) for t in image[x, H - 1 - r])
            y = kr * R + kg * G + kb * B
            ey[r, x], pb[r, x], pr[r, x] = y, 0.5 * (B - y) / (1.0 - kb), 0.5 * (R - y) / (1.0 - kr)
    dx, dy = {"center": (1, 1), "left": (0, 1), "topleft": (0, 0)}[siting]
    cpb = np.zeros((H // 2, W // 2)); cpr = np.zeros((H // 2, W // 2))
    for j in range(H // 2):
        rows = _taps(4 * j + dy, H)
        for i in range(W // 2):
            cols = _taps(4 * i + dx, W)
            cpb[j, i] = math.fsum(wr * wc * pb[r, c] for r, wr in rows for c, wc in cols)
            cpr[j, i] = math.fsum(wr * wc * pr[r, c] for r, wr in rows for c, wc in cols)
    s = 2.0 ** (bits - 8)
    top = 2.0 ** bits - 1.0
    if full_range:
        y, cb, cr = top * ey, top * cpb + 2.0 ** (bits - 1), top * cpr + 2.0 ** (bits - 1)
        return np.clip(y, 0.0, top), np.clip(cb, 0.0, top), np.clip(cr, 0.0, top)
    y, cb, cr = (219.0 * ey + 16.0) * s, (224.0 * cpb + 128.0) * s, (224.0 * cpr + 128.0) * s
    return np.clip(y, 16.0 * s, 235.0 * s), np.clip(cb, 16.0 * s, 240.0 * s), np.clip(cr, 16.0 * s, 240.0 * s)
