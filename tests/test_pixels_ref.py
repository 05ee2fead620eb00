"""Properties of the 8-bit pixel model (tests/pixels_ref.py), without a GPU: truncation is the reference's to_vec3u in the consumer's
orientation, rounding differs from it exactly where it must, and the dither keeps its fixed points, its range, its mean and its repeatability.

The 5 sigma rule: a two-LSB triangular dither makes the total quantisation error's variance 1/4 LSB^2 whatever the level, so a mean over N values has
sigma = 0.5 / sqrt(N) LSB.  The hash is fixed, so every result here is deterministic."""
import numpy as np

import pixels_ref as px
from digital_earth_amd.renderer import Renderer

F = np.float32


def _neighbours(x):
    x = np.asarray(x, F)
    return np.concatenate([np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))])


def _edge_image():
    """(W, H, 3) with every k/255 and its two f32 neighbours, values outside [0, 1], -0.0 and the infinities (no NaN: see the test)."""
    v = np.concatenate([_neighbours(np.arange(256, dtype=F) / F(255.0)), np.array([-0.0, -1e-30, -1.0, -3e38, 1.0 + 2.0 ** -23, 1.5, 3e38, np.inf, -np.inf, 1e-45], F)])
    v = np.resize(v, 16 * 56 * 3)
    return v.reshape(16, 56, 3)


def test_truncate_is_to_vec3u_in_the_consumers_orientation():
    rng = np.random.default_rng(1)
    for img in (rng.uniform(-0.2, 1.2, (48, 24, 3)).astype(F), _edge_image()):
        want = Renderer.to_vec3u(img).transpose(1, 0, 2)[::-1]
        for ch in (3, 4):
            got = px.pack(img, channels=ch)
            assert got.dtype == np.uint8 and got.shape == (img.shape[1], img.shape[0], ch)
            assert (got[..., :3] == want).all()
            assert ch == 3 or (got[..., 3] == 255).all()
    # a NaN is 0 by the model (the cast of a NaN that to_vec3u performs is not defined, so it is not the yardstick there)
    assert (px.pack(np.full((16, 8, 3), np.nan, F)) [..., :3] == 0).all()


def test_round_and_truncate_differ_exactly_where_the_fraction_is_a_half_or_more():
    rng = np.random.default_rng(2)
    t = np.concatenate([rng.uniform(-0.1, 1.1, 20000).astype(F), _edge_image().ravel(), (np.arange(255, dtype=F) + F(0.5)) / F(255.0)])
    s = px.scaled(t)
    lo, hi = px.quantise(t, "truncate"), px.quantise(t, "round")
    frac = s - np.floor(s)                                   # exact in f32: s < 2^8
    assert ((hi != lo) == (frac >= F(0.5))).all()
    assert ((hi - lo)[frac >= F(0.5)] == 1).all() and (lo == np.floor(s)).all()
    assert (frac >= F(0.5)).any() and (frac < F(0.5)).any()


def test_dither_fixed_points_and_range():
    rng = np.random.default_rng(3)
    t = np.concatenate([rng.uniform(-0.1, 1.1, 50000).astype(F), _edge_image().ravel(), _neighbours(np.array([0.0, 1.0 / 255, 254.0 / 255, 1.0], F)), np.array([np.nan], F)])
    idx = rng.integers(0, 2 ** 32, t.size, dtype=np.uint64).astype(np.uint32)
    for seed, phase in ((0, 0), (12345, 1), (0xffffffff, 77)):
        q = px.quantise(t, "dither", seed, phase, idx)
        s = px.scaled(t)
        with np.errstate(invalid="ignore"):
            assert (q[~(t > 0)] == 0).all()                  # exact 0, -0.0, negatives, -inf and NaN
            assert (q[t >= 1] == 255).all()                  # 1, above 1 and +inf
        assert q.min() >= 0 and q.max() <= 255
        assert np.abs(q - np.floor(s + F(0.5)).astype(np.int64)).max() <= 1


def test_dither_is_unbiased_over_phases():
    N = 4096
    bound = 5 * 0.5 / np.sqrt(N)
    rng = np.random.default_rng(4)
    s_want = np.concatenate([np.arange(1, 255, 11, dtype=np.float64), [1.0, 254.0, 1.25, 253.75, 127.5, 128.0], rng.uniform(1.0, 254.0, 40)])
    t = (s_want / 255.0).astype(F)
    s = px.scaled(t).astype(np.float64)
    assert (s >= 1.0).all() and (s <= 254.0).all()
    phases = np.arange(N)[:, None]
    for seed, pixel in ((0, 0), (2024, (37 * 208 + 101) * 4 + 1)):
        idx = np.full((1, t.size), pixel, np.uint32)
        q = px.quantise(t[None, :], "dither", seed, phases, idx)      # the restatement itself, every phase at once: (N, levels)
        assert q.shape == (N, t.size)
        for p in (0, 1, N - 1):                                       # broadcasting over the phases is what a call per phase gives
            assert (q[p] == px.quantise(t, "dither", seed, p, idx[0])).all()
        err = q.mean(axis=0) - s
        assert np.abs(err).max() <= bound, (seed, float(np.abs(err).max()), bound, s[np.abs(err) > bound])


def test_animate_off_repeats_and_on_changes_the_pattern():
    rng = np.random.default_rng(5)
    img = rng.uniform(0.0, 1.0, (32, 16, 3)).astype(F)
    img[:4] = 0.0
    img[4:8] = 1.0
    img[8:10] = 7.0
    a = px.pack(img, 4, "dither", seed=9, phase=0)
    assert (a == px.pack(img, 4, "dither", seed=9, phase=0)).all()       # animate = 0: the phase is 0 at every conversion
    b = px.pack(img, 4, "dither", seed=9, phase=1)
    c = px.pack(img, 4, "dither", seed=9, phase=2)
    inner = np.s_[:, 10:, :3]
    assert (a[inner] != b[inner]).mean() > 0.2 and (b[inner] != c[inner]).mean() > 0.2
    for o in (a, b, c):
        assert (o[:, :4, :3] == 0).all() and (o[:, 4:10, :3] == 255).all() and (o[..., 3] == 255).all()
    assert (px.pack(img, 4, "dither", seed=10, phase=0)[inner] != a[inner]).any()


def test_a_slow_ramp_bands_when_truncated_and_does_not_when_dithered():
    W, H = 256, 64
    s_want = 100.0625 + np.arange(W) / 8.0                   # 1/8 LSB per pixel, never within 1/16 of an integer
    img = np.repeat(np.repeat((s_want / 255.0).astype(F)[:, None, None], H, axis=1), 3, axis=2)
    s = px.scaled(img[:, 0, 0]).astype(np.float64)
    assert np.abs(s - s_want).max() < 1e-4
    flat = px.pack(img, 3, "truncate")
    assert (flat == flat[0:1]).all()
    row = flat[0, :, 0].astype(int)
    assert (row.reshape(-1, 8) == row[::8, None]).all() and (np.diff(row[::8]) == 1).all()      # runs of 8 equal values, one level apart: bands
    d = px.pack(img, 3, "dither", seed=1).astype(np.float64)              # (H, W, 3)
    bound = 5 * 0.5 / np.sqrt(64)
    blocks = d.reshape(H // 8, 8, W // 8, 8, 3).mean(axis=(1, 3))       # (H / 8, W / 8, 3)
    want = s.reshape(W // 8, 8).mean(axis=1)
    assert np.abs(blocks - want[None, :, None]).max() <= bound
    assert np.abs(flat.astype(np.float64).reshape(H // 8, 8, W // 8, 8, 3).mean(axis=(1, 3)) - want[None, :, None]).max() > 0.45      # truncation sits half a level low
