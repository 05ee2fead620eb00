"""Properties of the float64 restatement of the denoiser's filter (tests/denoise_f64.py) — what the GPU filter is held to (tests/test_gpu_denoise.py)."""
import numpy as np

import denoise_f64 as dn


def _guides(W, H, rng, land=True):
    g = np.zeros((W, H, 9))
    g[..., 0] = 1.0 if land else 0.0
    g[..., 1] = 1.0e6 + 1.0e3 * np.arange(W)[:, None] + 500.0 * np.arange(H)[None, :]
    n = np.zeros((W, H, 3)); n[..., 2] = 1.0
    n[..., 0] = 0.01 * rng.standard_normal((W, H))
    g[..., 2:5] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    g[..., 5:8] = 0.3
    g[..., 8] = 0.8
    return g


def test_constant_image_is_a_fixed_point():
    rng = np.random.default_rng(1)
    W, H = 32, 24
    mean = np.broadcast_to(np.array([0.2, 0.5, 0.1]), (W, H, 3)).copy()
    var = rng.uniform(0.0, 0.01, (W, H))
    g = _guides(W, H, rng)
    g[..., 5:8] = rng.uniform(0, 1, (W, H, 3))      # edges in the guides do not move a constant image either
    c, _ = dn.denoise(mean, var, g, levels=5, sigma_l=4.0)
    assert np.abs(c - mean).max() < 1e-12


def test_weights_are_normalised_and_non_negative():
    rng = np.random.default_rng(2)
    W, H = 24, 16
    col = rng.uniform(0, 1, (W, H, 3))
    var = rng.uniform(0, 0.05, (W, H))
    g = _guides(W, H, rng)
    g[: W // 2, :, 0] = 0.0
    for step in (1, 2, 4):
        _, _, taps = dn.atrous_level(col, var, g, step, 4.0, return_weights=True)
        s = sum(taps)
        assert np.abs(s - 1.0).max() < 1e-12
        assert min(t.min() for t in taps) >= 0.0
        # the centre tap keeps at least its kernel weight over the largest possible sum (1)
        assert taps[12].min() >= (0.375 ** 2) - 1e-12


def test_variance_recursion():
    """var_out = sum((w k)^2 v_q) / (sum w k)^2: with the normalised weights, the sum of their squares times the tap variances."""
    rng = np.random.default_rng(3)
    W, H = 20, 16
    col = rng.uniform(0, 1, (W, H, 3))
    var = rng.uniform(0, 0.05, (W, H))
    g = _guides(W, H, rng)
    c, v, taps = dn.atrous_level(col, var, g, 2, 4.0, return_weights=True)
    want = np.zeros((W, H))
    k = 0
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            vq, m = dn._shift(var, 2 * dx, 2 * dy)
            want += taps[k] ** 2 * np.where(m, vq, 0.0)
            k += 1
    assert np.abs(v - want).max() <= 1e-12 * max(1.0, want.max())
    # filtering never raises the variance above the input's largest (convex combination with squared weights)
    assert v.max() <= var.max() + 1e-15


def test_zero_variance_leaves_a_non_flat_image_unchanged():
    rng = np.random.default_rng(4)
    W, H = 32, 16
    level = 0.1 + 0.9 * rng.permutation(W * H).reshape(W, H) / (W * H)      # luminances at least 1.7e-3 apart: every luminance term is >= 1700
    col = level[..., None] * rng.uniform(0.5, 1.0, (1, 1, 3))
    col *= (level / dn.lum(col))[..., None]
    var = np.zeros((W, H))
    c, v = dn.denoise(col, var, _guides(W, H, rng), levels=5, sigma_l=4.0)
    assert np.abs(c - col).max() < 1e-12
    assert np.abs(v).max() == 0.0


def test_noise_is_reduced_on_a_flat_surface():
    rng = np.random.default_rng(5)
    W, H = 64, 32
    truth = np.broadcast_to(np.array([0.3, 0.3, 0.3]), (W, H, 3))
    sigma = 0.05
    noisy = truth + sigma * rng.standard_normal((W, H, 1))
    var = np.full((W, H), sigma * sigma)
    c, v = dn.denoise(noisy, var, _guides(W, H, rng), levels=5)
    assert np.sqrt(((c - truth) ** 2).mean()) < 0.5 * sigma
    assert v.mean() < 0.25 * sigma * sigma


def test_temporal_variance_rule():
    rng = np.random.default_rng(6)
    W, H, n = 8, 8, 16
    x = rng.uniform(0, 1, (n, W, H, 3))
    s1 = x.sum(0)
    s2 = (x * x).sum(0)
    mean, var = dn.prep_temporal(s1, s2, n)
    sd = x.std(0, ddof=1)
    assert np.allclose(mean, x.mean(0))
    assert np.allclose(var, (sd @ dn.LUM) ** 2 / n)
    _, var3 = dn.prep_temporal(s1, s2, 3)
    assert np.isnan(var3).all()
