"""The restatement of the bloom (tests/bloom_ref.py) checked on its own, without a GPU: threshold 0 passes the mean through bit for bit, the number of
levels used, the glow of interior impulses (its support, its exact zeros, the energy it conserves), and pixels that are not light (NaN, Inf, negative)
leaving every other pixel as if they were black."""
import numpy as np

import bloom_ref as bl


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scene(W, H, seed=3):
    rng = np.random.default_rng(seed)
    Y = np.exp2(rng.uniform(-30.0, 10.0, (W, H, 1)))
    return (Y * rng.uniform(-0.6, 2.0, (W, H, 3))).astype(np.float32)


def test_threshold_zero_gives_the_mean_bit_for_bit():
    sums = _scene(32, 16)
    for spp in (1, 7):
        m = bl.mean_of(sums, spp)
        b = bl.bright(m, threshold=0.0, knee=0.5, clamp=0.0)
        with np.errstate(all="ignore"):
            Y = (np.float32(0.2126) * m[..., 0] + np.float32(0.7152) * m[..., 1]) + np.float32(0.0722) * m[..., 2]
        lit = Y > 0
        assert lit.any() and (~lit).any()                     # the chroma range makes some luminances negative
        assert (_bits(b[lit]) == _bits(m[lit])).all()
        assert (b[~lit] == 0).all()
    # the knee is inert at threshold 0, whatever its value
    assert (_bits(bl.bright(m, 0.0, 1.0, 0.0)) == _bits(b)).all()


def test_threshold_knee_and_clamp_by_hand():
    m = np.array([[[0.1, 0.1, 0.1], [0.3, 0.3, 0.3], [1.0, 1.0, 1.0], [8.0, 8.0, 8.0]]], np.float32)
    b = bl.bright(m, threshold=0.3, knee=0.5, clamp=2.0)
    with np.errstate(all="ignore"):
        Y = (np.float32(0.2126) * m[..., 0] + np.float32(0.7152) * m[..., 1]) + np.float32(0.0722) * m[..., 2]
        Yb = (b[..., 0] / m[..., 0]) * Y
    assert b[0, 0, 0] == 0.0                                  # under threshold - knee: nothing
    assert 0.0 < Yb[0, 1] < 0.3 * 0.5                         # on the threshold: inside the knee
    assert abs(Yb[0, 2] - (Y[0, 2] - np.float32(0.3))) < 1e-6  # above the knee: Y - t
    assert abs(Yb[0, 3] - 2.0) < 1e-6                         # clamped
    assert (b >= 0).all() and (b <= m).all()


def test_levels_used():
    assert bl.levels_used(16, 8, 6) == 2
    assert bl.levels_used(16, 8, 1) == 1
    assert bl.levels_used(1920, 1080, 10) == 10
    assert bl.levels_used(1920, 1080, 6) == 6
    assert bl.levels_used(80, 56, 6) == 5
    assert bl.level_sizes(80, 56, 5) == [(80, 56), (40, 28), (20, 14), (10, 7), (5, 4), (3, 2)]
    assert bl.level_sizes(16, 8, 2)[-1] == (4, 2)
    for W, H in ((16, 8), (64, 64), (208, 120), (3840, 2160)):
        L = bl.levels_used(W, H, 10)
        assert L >= 1 and min(bl.level_sizes(W, H, L)[-1]) >= 2
        assert L == 10 or min(bl.level_sizes(W, H, L + 1)[-1]) < 2


def test_interior_impulses_keep_their_energy_and_their_support():
    W = H = 64
    sums = np.zeros((W, H, 3), np.float32)
    sums[31, 32] = (3.0, 2.0, 1.0)
    sums[32, 31] = (0.5, 4.0, 0.25)
    out, G, b = bl.bloom(sums, 1, intensity=0.4, levels=3)
    assert bl.levels_used(W, H, 3) == 3
    m = bl.mean_of(sums, 1)
    assert (_bits(b) == _bits(m)).all()
    # the two-pixel border ring of the glow is exactly zero, and so is everything further than 15 pixels from the impulses
    ring = np.ones((W, H), bool)
    ring[2:-2, 2:-2] = False
    assert (G[ring] == 0).all()
    lit = np.argwhere((G != 0).any(axis=-1))
    assert lit[:, 0].min() >= 31 - 15 and lit[:, 0].max() <= 32 + 15 and lit[:, 1].min() >= 31 - 15 and lit[:, 1].max() <= 32 + 15
    assert lit[:, 0].max() - lit[:, 0].min() >= 20            # and it is wide
    # energy: the weights are exact binary fractions that sum to 1, only rounding deviates
    for c in range(3):
        want = m[..., c].astype(np.float64).sum()
        assert abs(out[..., c].astype(np.float64).sum() - want) <= 1e-6 * want
        assert abs(G[..., c].astype(np.float64).sum() - want) <= 1e-6 * want
    # level 0 is not blended in: the glow at an impulse is far below the impulse
    assert G[31, 32, 0] < 0.2 * m[31, 32, 0]
    # intensity 0 is the mean, intensity 1 is the glow (plus the rounding of m + (G - m))
    assert (_bits(bl.bloom(sums, 1, intensity=0.0, levels=3)[0]) == _bits(m)).all()
    assert np.allclose(bl.bloom(sums, 1, intensity=1.0, levels=3)[0], G, rtol=0, atol=1e-6)


def test_a_constant_image_stays_constant():
    sums = np.full((48, 24, 3), 7 * 0.25, np.float32)
    out, G, b = bl.bloom(sums, 7, intensity=0.3)
    assert (G == 0.25).all() and (out == 0.25).all()          # every weight set sums to 1 exactly, clamped edges included


def test_pixels_that_are_not_light_leave_the_others_as_if_they_were_black():
    W, H = 32, 24
    rng = np.random.default_rng(8)
    sums = (np.exp2(rng.uniform(-6.0, 3.0, (W, H, 1))) * rng.uniform(0.5, 1.5, (W, H, 3))).astype(np.float32)
    bad = [(0, 0), (5, 7), (31, 23), (16, 12), (17, 12), (9, 20)]
    values = [(np.nan, 1, 1), (np.inf, 1, 1), (-np.inf, 0, 0), (-1, -2, -3), (np.inf, -np.inf, 0), (1, np.nan, np.nan)]
    dirty, black = sums.copy(), sums.copy()
    for (i, j), v in zip(bad, values):
        dirty[i, j] = v
        black[i, j] = 0.0
    for kw in (dict(), dict(threshold=0.3, knee=0.5, clamp=2.0, intensity=0.4)):
        got, G, b = bl.bloom(dirty, 2, **kw)
        want, G0, b0 = bl.bloom(black, 2, **kw)
        assert np.isfinite(G).all() and (_bits(G) == _bits(G0)).all() and (_bits(b) == _bits(b0)).all()
        mask = np.ones((W, H), bool)
        for i, j in bad:
            mask[i, j] = False
        assert (_bits(got[mask]) == _bits(want[mask])).all()
        assert np.isfinite(got[mask]).all()


def test_tile_counts_divide_like_the_display():
    W, H = 16, 8
    sums = np.full((W, H, 3), 6.0, np.float32)
    counts = np.full((W, H), 3, np.int32)
    counts[8:, :] = 6
    m = bl.mean_of(sums, counts)
    assert (m[:8] == 2.0).all() and (m[8:] == 1.0).all()
    out, G, b = bl.bloom(sums, counts)
    assert (_bits(b) == _bits(m)).all() and out.dtype == np.float32 and out.shape == (W, H, 3)
