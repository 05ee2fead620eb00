"""The local exposure's numpy float32 restatement (tests/local_exposure_ref.py, which the GPU equals bit for bit with the device's logarithm and power
injected) against the float64 statement of DESIGN.md §15 (tests/local_exposure_f64.py), and three properties of that statement.  No GPU.  Here the
restatement is given numpy's float32 `log` and `exp2`.

The bound (tests/local_exposure_f64_cases.py: `Base`, `compare`).  u = 2^-24; every f32 operation returns its exact result times (1 + d), |d| <= u.
Valid pixels of the inputs have non-negative channels and Y > 1e-6, the others are invalid by construction (Y <= 0, not finite, or 1e-9), so validity
is the same decision in both precisions and `D.y > 0` (a sum of exact binary fractions of 0s and 1s) is too.  Lam = the largest |l| of the image (<= 24).

  * l = log(Y) LOG2E.  Y: three products, two sums of non-negative terms over m: 4u relative, 4u log2(e) in l.  A logarithm good to k ulps (numpy's
    float32 log documents up to 4; 1 ulp <= 2u relative) of a value <= Lam ln 2, LOG2E's own rounding and the product:
    e_0 = 4u log2(e) + (2k + 2) u Lam.
  * Down, both components, weights >= 0 summing to 1.  Every partial value of the first component is at most Lam times the matching one of the second,
    so the six rounded operations per level of §12's tent (tests/test_bloom_f64.py) cost 6u Lam y per level in x and 6u y in y, on top of e_0 y carried
    along: dx_l <= (e_0 + 6 l u Lam) y_l, dy_l <= 6 l u y_l, and the guide x / y, one more operation: e_g(l) = e_0 + (12 l + 1) u Lam; e_g(0) = e_0
    (l 1 / 1).  No pattern of invalid pixels enters: the errors scale with the weight y itself.
  * Up.  B(p) = sum_t w_t B_t with w_t = k_t r_t / sum k r: a convex combination, so the taps' own errors pass on with their weights.  A relative error
    eps_t of k_t r_t moves B by sum_t w_t eps_t (B_t - B(p)) to first order: the normalisation takes the common part out.  r = 1 / (1 + a^2),
    a = (g - g_t) inv_sigma: the guides move a by (e_g(l) + e_g(l+1)) / sigma and inv_sigma, the difference and the product by 3u |a|;
    dr / r = 2 a da / (1 + a^2), and 2 a^2 / (1 + a^2) <= 2, so eps_t <= rho_t = 2 |a_t| / (1 + a_t^2) (e_g(l) + e_g(l+1)) / sigma + 9u (6u, the square,
    the sum, the quotient).  k r, its product with B_t, three sums each in `num` and `den` and the quotient: 10u max_t |B_t|.
    E_l(p) = sum_t w_t (E_{l+1}(t) + rho_t |B_t - B(p)|) + 10u max_t |B_t|, E_L = e_g(L), evaluated on the float64 statement's own taps.
  * mid = log(key / scale) LOG2E: e_mid = u log2(e) + (2k + 2) u |mid|.
  * ev = -(s (B - mid)) clamped: s (E_0 + e_mid) + 3u |ev|.  The gain 2^ev: ln 2 times that, plus the power's own relative error p (numpy's float32
    exp2: 4 ulps, 8u); m g: u; the input mean is given in f32: no division.  |out - out64| <= 1.01 |out64| (ln 2 (s (E_0 + e_mid) + 3u |ev|) + p + 2u);
    1.01 covers the products of two errors (rho is at most a few 1e-3).
  * Decisions.  A pixel is left out where the float64 |B - mid| <= 1.01 (E_0 + e_mid) (only if highlights != shadows: otherwise nothing is chosen) or
    ||raw ev| - max_ev| <= s times that + 3u max_ev (only if max_ev > 0 and s > 0: otherwise ev is 0 in both and the output must equal the input
    exactly).  The share of valid pixels left out is asserted below 1 % in every case.

Largest measured ratio to the bound 0.092, largest excluded share 0.06 % (printed per size)."""
import itertools

import numpy as np
import pytest

import bloom_f64 as b64
import local_exposure_f64 as x64
import local_exposure_ref as lx
from local_exposure_f64_cases import LEVELS, SIGMAS, SIZES, U, Base, compare, inputs, settings

NUMPY_LOG_ULPS, NUMPY_EXP2_REL = 4, 8 * U


def log32(x):
    return np.log(np.asarray(x, dtype=np.float32))


def pow2_32(e):
    return np.exp2(np.asarray(e, dtype=np.float32))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("size", SIZES)
def test_restatement_within_the_derived_bound(size):
    W, H = size
    worst, share = 0.0, 0.0
    for name, mean in inputs(W, H).items():
        m32 = lx.mean_of(mean, 1)
        l32, valid32 = lx.log_luminance(m32, log32)
        made = {}
        for sigma, levels in itertools.product(SIGMAS, LEVELS):
            L = len(b64.plan(W, H, levels)) - 1
            assert lx.levels_used(W, H, levels) == L
            if (sigma, L) not in made:
                made[(sigma, L)] = Base(mean, sigma, levels, NUMPY_LOG_ULPS)
            base = made[(sigma, L)]
            assert (valid32 == base.valid).all()
            B32 = lx.base(l32, valid32, sigma, levels)
            e_b = np.abs(B32 - base.B)[base.valid] / base.E[base.valid]
            assert e_b.max() <= 1.01, (name, sigma, levels, e_b.max())             # the base itself, no decision between
            worst = max(worst, float(e_b.max()))
            for k, (hi, lo, max_ev, scale) in enumerate(settings()):
                kw = dict(highlights=hi, shadows=lo, max_ev=max_ev)
                g = lx.gain(B32, valid32, lx.anchor(scale, 0.18, log32), hi, lo, max_ev, pow2_32)
                out = np.where(valid32[..., None], m32 * g[..., None], m32).astype(np.float32)
                if k % 17 == 0:                                                        # the pieces above are the restatement's own composition
                    whole = lx.local_exposure(mean, 1, scale, sigma=sigma, levels=levels, log=log32, pow2=pow2_32, **kw)[0]
                    assert ((_bits(whole) == _bits(out)) | np.isnan(whole)).all()
                r, s = compare(out, base, scale, kw, NUMPY_EXP2_REL, (name, sigma, levels, kw, scale))
                worst, share = max(worst, r), max(share, s)
    print("local exposure %dx%d: largest |ref - f64| / bound = %.4f, largest excluded share = %.4f" % (W, H, worst, share))


# ---------------------------------------------------------------- properties of the float64 statement
@pytest.mark.parametrize("size", [(48, 40), (80, 56)])
def test_without_range_weights_the_way_up_is_the_blooms_up_operator(size):
    """sigma = 1e6 and every pixel valid: r = 1 to 1e-9, every weight counts, and B_0 = (Ux_1 .. Ux_L)(Dx_L .. Dx_1) l (...)^T, which is §12's P at
    spread = 1 applied to l.  With invalid pixels the same holds per level for the pair: up(on B) / up(on)."""
    W, H = size
    mean = inputs(W, H)["random"]
    l, valid, _ = x64.log_luminance(mean)
    assert valid.all()
    for levels in LEVELS:
        B, _, L = x64.base(l, valid, 1e6, levels)
        assert np.abs(B - b64.apply(b64.factors(W, H, levels, 1.0), l)).max() < 1e-8
    l, valid, _ = x64.log_luminance(inputs(W, H)["dirty"])
    D = x64.pyramid(l, valid, 6)
    (g1, on1), (g0, on0) = x64.guide(D[2]), x64.guide(D[1])
    B1 = np.where(on1, np.sin(np.arange(g1.size).reshape(g1.shape)), 0.0)
    Ux, Uy = b64.up_matrix(g0.shape[0], g1.shape[0]), b64.up_matrix(g0.shape[1], g1.shape[1])
    B0, _ = x64.up(g0, on0, g1, on1, B1, 1e6)
    num, den = Ux @ (on1 * B1) @ Uy.T, Ux @ on1.astype(float) @ Uy.T
    assert not on0.all() and np.abs(B0 - num / np.where(den > 0, den, 1.0))[on0].max() < 1e-8


@pytest.mark.parametrize("size", [(48, 40), (80, 56)])
def test_the_base_of_a_step_keeps_each_sides_level_up_to_the_edge(size):
    """Two levels 4 stops apart, sigma = 0.25: the step is 16 sigma.  One level: a coarse sample astride the edge holds the other side with a share q, so
    its value and its guide are off by q step and its range weight is 1 / (1 + (q step / sigma)^2); q step / (1 + (q step / sigma)^2) <= sigma / 2 for
    every q.  Next to a tap of the sample's own side, which weighs at least a third of it in space (1/4 against 3/4), it moves the base by at most
    3 sigma / 2 = 3/32 of the step, whatever the step: the edge is kept right up to its two columns, where the plain `up` (sigma = 1e6) is off by 3/8
    of the step.  Every further level starts from coarser mixtures (the coarsest guide of a small image spans both sides), which is the halo DESIGN §15
    quotes; there the range weights still at least halve the plain pyramid's error."""
    W, H = size
    mean = np.where(np.arange(W)[:, None, None] < W // 2 + 1, np.float32(0.02), np.float32(0.32)) * np.ones((W, H, 3), np.float32)
    l, valid, _ = x64.log_luminance(mean)
    side = np.where(np.arange(W)[:, None] < W // 2 + 1, l[0, 0], l[-1, 0]) * np.ones((1, H))
    step = l[-1, 0] - l[0, 0]
    assert abs(step - 4.0) < 1e-6
    off = {(sigma, levels): np.abs(x64.base(l, valid, sigma, levels)[0] - side) for sigma in (0.25, 1e6) for levels in (1, 2)}
    assert off[(0.25, 1)].max() <= 1.5 * 0.25 and off[(0.25, 1)].max() < step / 10
    assert abs(off[(1e6, 1)].max() - 3 * step / 8) < 1e-6
    assert off[(0.25, 2)].max() < off[(1e6, 2)].max() / 2


def test_invalid_pixels_change_no_other_pixels_base():
    W, H = 48, 40
    dirty = inputs(W, H)["dirty"]
    l, valid, _ = x64.log_luminance(dirty)
    other = dirty.copy()
    other[~valid] = (-3.0, np.nan, np.inf)                                            # other values that are not light
    l2, valid2, _ = x64.log_luminance(other)
    assert (valid2 == valid).all() and not valid.all()
    for sigma in SIGMAS:
        B, B2 = x64.base(l, valid, sigma, 6)[0], x64.base(l2, valid2, sigma, 6)[0]
        assert (B[valid] == B2[valid]).all()
    # and a valid pixel among them is not dragged towards 0: its base is a mean of valid neighbours' l
    B = x64.base(l, valid, 1.0, 6)[0]
    assert B[valid].min() >= l[valid].min() - 1e-12 and B[valid].max() <= l[valid].max() + 1e-12
