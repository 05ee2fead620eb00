"""Inputs, settings, the derived bound and the comparison that tests/test_local_exposure_f64.py (the float32 restatement, CPU) and
tests/test_gpu_local_exposure_f64.py (the device) share.  The derivation of the bound is in the docstring of tests/test_local_exposure_f64.py."""
import itertools

import numpy as np

import local_exposure_f64 as x64

U = 2.0 ** -24
SIZES = [(16, 8), (48, 40), (80, 56), (208, 120)]
LEVELS = (1, 2, 6, 10)
STRENGTHS, SIGMAS, MAX_EVS, SCALES = (0.0, 0.25, 1.0), (0.25, 1.0, 1e6), (0.0, 2.0), (0.25, 1.0, 8.0)
CAP = 0.01
SECOND_ORDER = 1.01
LOG2E = float(np.log2(np.e))

_INPUTS = {}


def spots(W, H):
    """The four corners, the middle of each edge, one pixel inside each edge, the interior."""
    return [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2 - 1, H - 1), (0, H // 2), (W - 1, H // 2 - 1),
            (W // 3, 1), (W // 3 + 1, H - 2), (1, H // 3), (W - 2, H // 3 + 1), (W // 2, H // 2), (W // 3, H // 3), (W // 3 + 1, H // 3)]


def inputs(W, H):
    """name -> (W, H, 3) float32 means, made once per size.  A pixel's luminance is above 1e-6 or it is not valid by construction."""
    if (W, H) in _INPUTS:
        return _INPUTS[(W, H)]
    rng = np.random.default_rng(1500 * W + H)
    random = (np.exp2(rng.uniform(-9.0, 3.0, (W, H, 1))) * rng.uniform(0.6, 1.4, (W, H, 3))).astype(np.float32)
    impulses = np.full((W, H, 3), 2.0 ** -6, np.float32)
    for k, (i, j) in enumerate(spots(W, H)):
        impulses[i, j] = (40.0 + k, 25.0 - k, 10.0 + 3 * k)
    rectangle = np.full((W, H, 3), 0.01, np.float32)
    rectangle[:max(W // 3, 3), :max(H // 2, 3)] = (6.0, 5.0, 3.0)              # touches the left and the top border
    constant = np.full((W, H, 3), 0.4, np.float32)
    dirty = random.copy()
    dirty[W // 4:W // 4 + max(W // 4, 3), H // 4:H // 4 + max(H // 4, 3)] = 0.0      # a block of black space
    k = rng.permutation(W * H)[:max(W * H // 20, 9)]
    values = np.array([(0, 0, 0), (-1.0, -2.0, -0.5), (np.nan, 1, 1), (np.inf, 1, 1), (-np.inf, 0, 0), (1e-9, 1e-9, 1e-9), (1, np.nan, np.nan),
                       (np.inf, np.inf, np.inf), (np.inf, -np.inf, 0)], np.float32)
    dirty.reshape(-1, 3)[k] = values[np.arange(len(k)) % len(values)]
    _INPUTS[(W, H)] = dict(random=random, impulses=impulses, rectangle=rectangle, constant=constant, dirty=dirty)
    return _INPUTS[(W, H)]


class Base:
    """The float64 base of one (mean, sigma, levels) with its error figure E for a float32 evaluation whose logarithm is good to `log_ulps` ulps."""

    def __init__(self, mean, sigma, levels, log_ulps):
        self.m = np.asarray(mean, dtype=np.float64)
        self.l, self.valid, Y = x64.log_luminance(self.m)
        with np.errstate(all="ignore"):
            # the one decision on a pixel alone is the same in both precisions by construction
            assert (Y[self.valid] > 1e-6).all() and (self.m[self.valid] >= 0).all() and not ((Y > 2.0 ** -26) & ~self.valid & np.isfinite(Y)).any()
        self.lam = max(1.0, float(np.abs(self.l[self.valid]).max()))
        self.rel_log = (2 * log_ulps + 2) * U                            # the logarithm's ulps (1 ulp <= 2u relative), LOG2E's rounding, the product
        e0 = U * 4 * LOG2E + self.rel_log * self.lam
        self.B, self.E, self.L = x64.base(self.l, self.valid, sigma, levels, e_g=lambda lv: e0 + ((12 * lv + 1) * U * self.lam if lv else 0.0))


def compare(got, base, exposure_scale, kw, pow_rel, what):
    """Hold `got` (f32 output of the restatement or the device) to the float64 statement.  Returns (largest ratio to the bound, excluded share)."""
    m, valid, B = base.m, base.valid, base.B
    hi, lo, max_ev = (x64._s(kw.get(k, d)) for k, d in (("highlights", 0.5), ("shadows", 0.25), ("max_ev", 2.0)))
    mid = x64.anchor(exposure_scale, kw.get("key", 0.18))
    e_mid = U * LOG2E + base.rel_log * abs(mid)
    margin = SECOND_ORDER * (base.E + e_mid)
    ev, raw = x64.exposure(B, mid, hi, lo, max_ev)
    s = np.where(B > mid, hi, lo)
    near = np.zeros(B.shape, bool)
    if hi != lo:
        near |= np.abs(B - mid) <= margin                                 # the choice of the strength
    if max_ev > 0:
        near |= (s > 0) & (np.abs(np.abs(raw) - max_ev) <= s * margin + 3 * U * max_ev)      # the clamp
    share = float((near & valid).sum()) / max(int(valid.sum()), 1)
    assert share < CAP, (what, share)
    got = np.asarray(got, dtype=np.float64)
    keep = np.isnan(m[~valid])
    assert (np.isnan(got[~valid]) == keep).all() and (got[~valid][~keep] == m[~valid][~keep]).all(), what      # what is not light passes as it is
    use = valid & ~near
    with np.errstate(all="ignore"):
        want = m * np.exp2(ev)[..., None]
        bound = SECOND_ORDER * np.abs(want) * (np.log(2.0) * (s * (base.E + e_mid) + 3 * U * np.abs(ev)) + pow_rel + 2 * U)[..., None]
    if max_ev == 0 or (hi == 0 and lo == 0):
        assert (got[valid] == m[valid]).all(), what                       # ev is 0 in both: the gain is exactly 1
    ratio = np.abs(got - want)[use] / np.maximum(bound[use], 1e-300)
    ratio = np.where(np.abs(got - want)[use] == 0, 0.0, ratio)
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, (what, worst)
    return worst, share


def settings():
    """(highlights, shadows, max_ev, exposure_scale): everything that acts after the base."""
    return itertools.product(STRENGTHS, STRENGTHS, MAX_EVS, SCALES)
