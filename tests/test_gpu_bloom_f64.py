"""Bloom on the GPU against the float64 statement of DESIGN.md §12 (tests/bloom_f64.py) directly, with no float32 restatement in the loop: a change that
moves the kernels and tests/bloom_ref.py together still meets a yardstick written from the prose.  Inputs, bound and its derivation are those of
tests/test_bloom_f64.py; the device's operations are the restatement's, one for one, so the count of rounded operations is the same.

spp 1 and 3 (the division by the count is in), threshold 0 and 0.02, spread 0.7 and 1, levels 2 and 10, intensity 0.4, at 16x8, 48x40, 80x56 and 208x120;
and one adaptive frame at 48x40 whose per-tile counts the float64 statement divides by."""
import itertools

import numpy as np
import pytest

import bloom_f64 as b64
from test_bloom_f64 import SIZES, Statement, compare, factors, inputs

pytestmark = pytest.mark.gpu

TAUS = (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01)


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.mark.parametrize("size", SIZES)
def test_bloom_hdr_is_within_the_derived_bound_of_the_float64_statement(R, size):
    W, H = size
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    r.copy_textures()
    worst = 0.0
    for (name, sums), spp in itertools.product(inputs(W, H).items(), (1, 3)):
        r.upload_hdr(sums, spp)
        for t, spread, levels in itertools.product((0.0, 0.02), (0.7, 1.0), (2, 10)):
            st = Statement(sums, spp, factors(W, H, levels, spread), t, 0.5, 0.0)
            r.set_bloom(True, intensity=0.4, threshold=t, spread=spread, levels=levels)
            worst = max(worst, compare(r.fetch_bloom_hdr(), st, 0.4, (name, spp, t, spread, levels)))
    r.close()
    print("bloom on the device %dx%d: largest |gpu - f64| / bound = %.4f" % (W, H, worst))


def test_an_adaptive_frame_is_divided_by_its_tile_counts(R):
    W, H = 48, 40
    r = R.Renderer((W, H), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=11)
    r.set_fov(0.42)
    r.copy_textures()
    for tau in TAUS:
        r.reset_framebuffer()
        r.render_adaptive(tau, 32, min_spp=4, round_spp=4)
        counts = r.tile_spp()
        if len(np.unique(counts)) >= 2:
            break
    else:
        pytest.fail("no threshold of %s spreads the tile counts" % (TAUS,))
    per_pixel = np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1)
    hdr = r.fetch_hdr()
    r.set_bloom(True, intensity=0.4, threshold=0.02)
    got = r.fetch_bloom_hdr()
    r.close()
    fs = b64.factors(W, H, 6, 0.7)
    # a rendered frame's dimmest light pixels are what they are: a sum of non-negative terms is > 0 in both precisions while none is subnormal
    ratio = compare(got, Statement(hdr, per_pixel, fs, 0.02, 0.5, 0.0, y_min=2.0 ** -100), 0.4, "adaptive")
    whole = Statement(hdr, int(counts.max()), fs, 0.02, 0.5, 0.0, y_min=2.0 ** -100)
    assert (np.abs(got - whole.out(0.4)) > whole.bound()).any()              # the frame's largest count would give something else
    print("bloom on the device, adaptive 48x40: largest |gpu - f64| / bound = %.4f" % ratio)
