"""The output scaling (include/digital_earth_output_scale.h) restated in numpy, following the header line by line: the table of an
axis in double precision with its float32 correction, and the two float32 passes — along v first, then along u, a multiply and then an add per tap in
ascending order, the zero padding included, an axis of equal size a copy, the last pass that runs clamped.  The GPU equals `resample` bit for bit when
both use the same tables; the tables themselves meet the library's within a float32 ulp (two libms evaluate the Lanczos sine)."""
import math

import numpy as np

F = np.float32
FILTERS = ("box", "triangle", "mitchell", "lanczos3")
SUPPORT = (0.5, 1.0, 2.0, 3.0)
DEFAULTS = dict(size=None, filter="lanczos3", on=True)      # Renderer.set_output_scale's keywords
MAX_TAPS = 49


def _sinc(z):
    if z == 0.0:
        return 1.0
    p = math.pi * z
    return math.sin(p) / p


def kernel(f, t):
    """k(t) of filter number f, in double precision, with the header's expressions in the header's order."""
    at = abs(t)
    if f == 0:
        return 1.0
    if f == 1:
        return 1.0 - at if at < 1.0 else 0.0
    if f == 2:
        if at < 1.0:
            return (7.0 * at * at * at - 12.0 * at * at + 16.0 / 3.0) / 6.0
        if at < 2.0:
            return (-7.0 / 3.0 * at * at * at + 12.0 * at * at - 20.0 * at + 32.0 / 3.0) / 6.0
        return 0.0
    return _sinc(t) * _sinc(t / 3.0) if at < 3.0 else 0.0


def _filter_number(filter):
    return FILTERS.index(filter) if isinstance(filter, str) else int(filter)


def geometry(n_src, n_dst, filter):
    """(r, s, [x_j], [first_j], [count_j]) of an axis."""
    r = float(n_src) / float(n_dst)
    s = r if r > 1.0 else 1.0
    R = SUPPORT[_filter_number(filter)] * s
    xs, lo, cnt = [], [], []
    for j in range(n_dst):
        x = (float(j) + 0.5) * r - 0.5
        a, b = int(math.floor(x - R)) + 1, int(math.ceil(x + R)) - 1
        if b < a:
            a = b = int(math.floor(x + 0.5))
        xs.append(x); lo.append(a); cnt.append(b - a + 1)
    return r, s, xs, lo, cnt


def weights(n_src, n_dst, filter):
    """The table of one axis: (first, w) — first (n_dst,) int32, unclamped; w (n_dst, taps) float32, rows padded with zeros, every row summing to exactly
    1.0f when added in tap order in float32 (the last tap ahead of the padding is fl(1 - P), P the float32 sum of the taps before it)."""
    f = _filter_number(filter)
    r, s, xs, lo, cnt = geometry(n_src, n_dst, f)
    taps = max(cnt)
    assert 1 <= taps <= MAX_TAPS
    w = np.zeros((n_dst, taps), F)
    for j in range(n_dst):
        k = [kernel(f, (float(lo[j] + t) - xs[j]) / s) for t in range(cnt[j])]
        total = 0.0
        for v in k:
            total = total + v
        P = F(0.0)
        for t in range(cnt[j] - 1):
            w[j, t] = F(k[t] / total)
            P = F(P + w[j, t])
        w[j, cnt[j] - 1] = F(F(1.0) - P)
        assert F(P + w[j, cnt[j] - 1]) == F(1.0)
    return np.array(lo, np.int32), w


def row_sums(w):
    """The float32 sum of every row in tap order from 0.0f: what a constant image of 1.0 comes out as."""
    acc = np.zeros(w.shape[0], F)
    for t in range(w.shape[1]):
        acc = (acc + w[:, t]).astype(F)
    return acc


def clamp01(a):
    """t > 0 ? (t < 1 ? t : 1) : 0 — NaN and -0.0 give +0.0."""
    with np.errstate(invalid="ignore"):
        return np.where(a > 0, np.where(a < 1, a, F(1.0)), F(0.0)).astype(F)


def _pass(src, axis, table):
    """One pass along `axis` (0: u, 1: v) of a (·, ·, 3) float32 image."""
    first, w = table
    n = src.shape[axis]
    acc = None
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for t in range(w.shape[1]):
            idx = np.clip(first.astype(np.int64) + t, 0, n - 1)
            wt = w[:, t].astype(F)
            term = (wt[:, None, None] * src[idx]) if axis == 0 else (wt[None, :, None] * src[:, idx])
            term = term.astype(F)
            acc = (np.zeros_like(term) + term).astype(F) if acc is None else (acc + term).astype(F)
    return acc


def resample(image, size, filter="lanczos3", tables=None):
    """image (W, H, 3) float32 -> (ow, oh, 3) float32, size = (ow, oh).  tables = (table of the u axis, table of the v axis), each (first, w) as
    weights() returns (or the library's own, so that the comparison of images is independent of libm); None builds them here.  The table of an axis
    of equal size is not used."""
    image = np.ascontiguousarray(image, dtype=F)
    W, H = image.shape[:2]
    ow, oh = size
    if tables is None:
        tables = (weights(W, ow, filter) if ow != W else None, weights(H, oh, filter) if oh != H else None)
    out = image
    if oh != H:
        out = _pass(out, 1, tables[1])
    if ow != W:
        out = _pass(out, 0, tables[0])
    if ow != W or oh != H:
        out = clamp01(out)
    return np.ascontiguousarray(out, dtype=F)
