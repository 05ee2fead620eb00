"""The restatement of the local exposure (tests/local_exposure_ref.py) checked on its own, without a GPU: strengths 0 return the input bits, pixels that
are not light keep their bits and weigh nothing, a constant image gets one gain, the three channels share the gain, and the base stops at an edge —
a larger gain jump across it and a smaller halo beside it than the same pyramid without the range weights."""
import numpy as np

import local_exposure_ref as lx


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scene(W, H, seed=3):
    rng = np.random.default_rng(seed)
    return (np.exp2(rng.uniform(-10.0, 2.0, (W, H, 1))) * rng.uniform(0.6, 1.4, (W, H, 3))).astype(np.float32)


def test_levels_follow_the_blooms_rule():
    assert lx.levels_used(16, 8, 6) == 2 and lx.levels_used(16, 8, 1) == 1
    assert lx.levels_used(64, 32, 6) == 4 and lx.levels_used(80, 56, 6) == 5 and lx.levels_used(208, 120, 6) == 6
    assert lx.levels_used(1920, 1080, 10) == 10


def test_zero_strengths_return_the_input_bits():
    m = _scene(64, 32)
    out, g = lx.local_exposure(m, 1, 4.0, highlights=0.0, shadows=0.0)
    assert (g == 1).all() and (_bits(out) == _bits(m)).all()
    sums = (m * np.float32(3)).astype(np.float32)
    out, g = lx.local_exposure(sums, 3, 4.0, highlights=0.0, shadows=0.0)
    assert (_bits(out) == _bits(lx.mean_of(sums, 3))).all()


def test_pixels_that_are_not_light_keep_their_bits_and_weigh_nothing():
    W, H = 80, 56
    clean = _scene(W, H)
    spots = [(0, 0), (W - 1, H - 1), (W - 1, 3), (40, 28), (41, 28), (7, 55), (20, 20)]
    values = [(0, 0, 0), (-1, -2, -0.5), (np.nan, 1, 1), (np.inf, 1, 1), (1e-9, 1e-9, 1e-9), (-np.inf, 0, 0), (np.inf, np.inf, np.inf)]
    outs = []
    for shift in range(3):
        m = clean.copy()
        m[30:36, 10:17] = 0.0 if shift == 0 else (-3.0 if shift == 1 else np.nan)      # a block of black space, then the same block negative, then NaN
        for k, (i, j) in enumerate(spots):
            m[i, j] = values[(k + shift) % len(values)]
        out, g = lx.local_exposure(m, 1, 4.0)
        bad = np.zeros((W, H), bool)
        bad[30:36, 10:17] = True
        for i, j in spots:
            bad[i, j] = True
        nan = np.isnan(m)
        assert (np.isnan(out) == nan).all()
        assert (_bits(out)[bad] == _bits(m)[bad])[~nan[bad]].all()                     # their own bits
        assert (g[bad] == 1).all() and (g[~bad] != 1).any()
        outs.append((out, bad))
    for out, bad in outs[1:]:
        assert (_bits(out)[~bad] == _bits(outs[0][0])[~bad]).all()                     # no neighbour's output changes when their values change


def test_a_constant_image_gets_one_gain_clamped_at_max_ev():
    W, H = 64, 32
    scale = 4.0
    mid_lum = 0.18 / scale
    for k, highlights, max_ev in ((1.0, 0.5, 2.0), (3.0, 0.5, 2.0), (3.0, 1.0, 2.0), (6.0, 0.5, 2.0), (-2.0, 0.5, 2.0)):
        m = np.full((W, H, 3), mid_lum * 2.0 ** k, np.float32)
        out, g = lx.local_exposure(m, 1, scale, highlights=highlights, shadows=0.25, max_ev=max_ev)
        assert (g == g[0, 0]).all()
        strength = highlights if k > 0 else 0.25
        want = 2.0 ** float(np.clip(-strength * k, -max_ev, max_ev))
        assert abs(float(g[0, 0]) / want - 1.0) < 1e-5, (k, highlights, float(g[0, 0]), want)
    assert abs(float(lx.local_exposure(np.full((W, H, 3), mid_lum * 64.0, np.float32), 1, scale)[1][0, 0]) - 0.25) < 1e-6      # 6 stops x 0.5 = 3 EV, clamped at 2


def test_the_three_channels_share_the_gain():
    m = _scene(80, 56, seed=9)
    out, g = lx.local_exposure(m, 1, 4.0)
    assert (g != 1).mean() > 0.9
    for c in range(3):
        assert (_bits(out[..., c]) == _bits(m[..., c] * g)).all()


def edge_figures(sigma):
    """(gain jump across the edge, halo) of a vertical step of 4 stops at 64x32: the ratio of the gains of the two pixels adjoining the edge (>= 1), and
    the largest deviation, in stops, of a side's gain from that side's far-field gain (the gain of its outermost column)."""
    W, H = 64, 32
    m = np.empty((W, H, 3), np.float32)
    m[:W // 2] = 0.02
    m[W // 2:] = 0.32
    out, g = lx.local_exposure(m, 1, 4.0, sigma=sigma)      # anchor 0.045: the dark side is lifted, the bright side is held back
    row = g[:, H // 2].astype(np.float64)
    jump = row[W // 2 - 1] / row[W // 2]
    halo = max(np.abs(np.log2(row[:W // 2] / row[0])).max(), np.abs(np.log2(row[W // 2:] / row[-1])).max())
    return float(jump), float(halo)


def test_the_base_stops_at_an_edge():
    aware, blind = edge_figures(1.0), edge_figures(1e9)
    print("edge-aware (sigma = 1): gain jump %.4f, halo %.4f stops; not edge-aware (sigma = 1e9): gain jump %.4f, halo %.4f stops" % (aware + blind))
    assert aware[0] > blind[0]      # the gains of the two sides stay apart right up to the edge ...
    assert aware[1] < blind[1]      # ... and neither side's gain drifts towards the other's near it
    # an ideal base is flat on either side: the far-field gains are 2^(0.25 x 1.17) and 2^(-0.5 x 2.83), a jump of 3.26
    assert aware[0] > 1.0 and blind[1] > 0.0
