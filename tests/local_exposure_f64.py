"""A float64 statement of the local exposure (include/digital_earth_local_exposure.h), written from the prose: which pixels count, log2
luminance and its weight, the weighted pyramid down as dense per-axis operators (those of tests/bloom_f64.py: §15 takes sizes, clamping and filter from
§12), the joint-bilateral way back up as a plain loop over output samples, the anchor, the choice of strength, the clamp and the one gain.  numpy's
float64 log2 / exp2 throughout, no device math.  It shares no code with tests/local_exposure_ref.py, tests/bloom_ref.py or csrc/.

`base` can carry the first-order error propagation of its own loop along (see tests/test_local_exposure_f64.py for the derivation): given the error
e_g[l] of every level's guide it returns, per pixel, how far a float32 evaluation of the same definition may land from B.  That figure is a function of
the float64 statement and of the number format alone.

Arrays are (W, H, 3) in fetch_hdr's layout: axis 0 is x, axis 1 is y.  Settings enter as the `float` fields hold them."""
import numpy as np

import bloom_f64 as b64

FLT_MAX = float(np.finfo(np.float32).max)
Y_MIN = 2.0 ** -24
U = 2.0 ** -24


def _s(v):
    return float(np.float32(v))


def log_luminance(m):
    """(l, valid, Y): a pixel counts iff 2^-24 <= Y <= FLT_MAX; l = log2 Y there and 0 elsewhere."""
    Y = b64.luminance(np.asarray(m, dtype=np.float64))
    with np.errstate(all="ignore"):
        valid = (Y >= Y_MIN) & (Y <= FLT_MAX)
        l = np.where(valid, np.log2(np.where(valid, Y, 1.0)), 0.0)
    return l, valid, Y


def pyramid(l, valid, levels):
    """[D_0 .. D_L], D_l of shape (w_l, h_l, 2) = (sum of weights x l, sum of weights): §12's down operators on both components."""
    sizes = b64.plan(l.shape[0], l.shape[1], levels)
    D = [np.stack([np.where(valid, l, 0.0), valid.astype(np.float64)], axis=-1)]
    for (w, h) in sizes[:-1]:
        Dx, Dy = b64.down_matrix(w), b64.down_matrix(h)
        D.append(np.moveaxis(np.tensordot(Dy, np.tensordot(Dx, D[-1], axes=(1, 0)), axes=(1, 1)), 0, 1))
    return D


def guide(D):
    """(mean log luminance of the level, where it has any weight)."""
    on = D[..., 1] > 0
    return np.where(on, D[..., 0] / np.where(on, D[..., 1], 1.0), 0.0), on


def taps(n_fine, n_coarse):
    """Per fine index: (near, far) with near = x >> 1 and far = near - 1 (even x) or near + 1 (odd x), clamped to the coarse level."""
    x = np.arange(n_fine)
    near = x >> 1
    far = np.where(x % 2 == 0, near - 1, near + 1)
    return near, np.minimum(np.maximum(far, 0), n_coarse - 1)


def up(g, on, gc, onc, Bc, sigma, Ec=None, e_pair=0.0):
    """One level of the base: for every fine sample with weight, the four coarse taps (3/4 near, 1/4 far per axis) that have weight, each times
    r = 1 / (1 + a^2), a = (guide of the sample - guide of the tap) / sigma, normalised.  The loop runs over output columns x; each step handles the
    samples (x, 0 .. h-1) at once.  Returns (B, E): E is None unless Ec, the taps' error, is given; e_pair is the error of a guide difference."""
    w, h = g.shape
    xn, xf = taps(w, gc.shape[0])
    yn, yf = taps(h, gc.shape[1])
    B = np.zeros((w, h))
    E = None if Ec is None else np.zeros((w, h))
    for x in range(w):
        got = []
        for xi, kx in ((xn[x], 0.75), (xf[x], 0.25)):
            for ys, ky in ((yn, 0.75), (yf, 0.25)):
                a = (g[x] - gc[xi, ys]) / sigma
                wgt = np.where(onc[xi, ys], kx * ky / (1.0 + a * a), 0.0)
                got.append((wgt, Bc[xi, ys], a, None if Ec is None else Ec[xi, ys]))
        den = sum(t[0] for t in got)
        assert (den[on[x]] > 0).all()                         # the sample lies inside its (near, near) tap's footprint
        den = np.where(on[x], den, 1.0)
        B[x] = np.where(on[x], sum(t[0] * t[1] for t in got) / den, 0.0)
        if Ec is not None:
            e = 10 * U * np.max([np.abs(t[1]) * (t[0] > 0) for t in got], axis=0)
            for wgt, Bt, a, Et in got:
                rho = 2 * np.abs(a) / (1.0 + a * a) * e_pair / sigma + 9 * U
                e = e + wgt / den * (Et + rho * np.abs(Bt - B[x]))
            E[x] = np.where(on[x], e, 0.0)
    return B, E


def base(l, valid, sigma=1.0, levels=6, e_g=None):
    """(B_0, E_0).  B_L is the coarsest level's guide; every finer level comes from `up`; level 0's guide is l itself.  e_g(level) -> the error of that
    level's guide, or None for no error propagation."""
    D = pyramid(l, valid, levels)
    L = len(D) - 1
    sigma = _s(sigma)
    gc, onc = guide(D[L])
    B, E = gc, None if e_g is None else np.full(gc.shape, e_g(L))
    for lv in range(L - 1, -1, -1):
        g, on = guide(D[lv])
        B, E = up(g, on, gc, onc, B, sigma, E, 0.0 if e_g is None else e_g(lv) + e_g(lv + 1))
        gc, onc = g, on
    return B, E, L


def anchor(exposure_scale, key=0.18):
    """mid: the scene luminance that the display maps to the key, in stops."""
    return float(np.log2(_s(key) / _s(exposure_scale)))


def exposure(B, mid, highlights=0.5, shadows=0.25, max_ev=2.0):
    """(ev, raw): the strength is `highlights` where the base is above the anchor, else `shadows`; raw is ev before the clamp to +-max_ev."""
    raw = -(np.where(B > mid, _s(highlights), _s(shadows)) * (B - mid))
    return np.minimum(np.maximum(raw, -_s(max_ev)), _s(max_ev)), raw


def local_exposure(mean, exposure_scale, highlights=0.5, shadows=0.25, sigma=1.0, max_ev=2.0, key=0.18, levels=6):
    """(out, gain, B, valid).  One gain 2^ev for all three channels of a valid pixel; the others pass as they are."""
    m = np.asarray(mean, dtype=np.float64)
    l, valid, _ = log_luminance(m)
    B, _, _ = base(l, valid, sigma, levels)
    ev, _ = exposure(B, anchor(exposure_scale, key), highlights, shadows, max_ev)
    g = np.where(valid, np.exp2(ev), 1.0)
    with np.errstate(all="ignore"):
        return np.where(valid[..., None], m * g[..., None], m), g, B, valid
