"""Local exposure on the GPU against the float64 statement of DESIGN.md §15 (tests/local_exposure_f64.py) directly, through the test hook
`debug_local_exposure`, with no float32 restatement in the loop.  Inputs, bound, exclusion and the 1 % cap are those of
tests/test_local_exposure_f64.py.  The device's `de_log` and `de_pow` replace numpy's, and the bound is taken with their stated errors:
de_math.h gives its first-contract functions, `de_log` and `de_exp`, as good to 2 ulps for a general argument (DESIGN §2's 3.4e-7 is `de_log_unit`
on draws), so k = 2 in the logarithm's term, and `de_pow(2, ev) = de_exp(ev de_log(2))` is off by de_log(2)'s 4u and the product's u on an exponent
|ev| ln 2 <= 2 ln 2, 7u, plus de_exp's 4u: p = 11u.

Sizes 16x8, 48x40, 80x56, 208x120; sigma 0.25 and 1, levels 2 and 10, highlights / shadows (0.25, 1) and (1, 0.25), max_ev 2, exposure scale 1 and 8."""
import itertools

import numpy as np
import pytest

from local_exposure_f64_cases import SIZES, U, Base, compare, inputs

pytestmark = pytest.mark.gpu

DE_LOG_ULPS, DE_POW2_REL = 2, 11 * U


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.mark.parametrize("size", SIZES)
def test_hook_is_within_the_derived_bound_of_the_float64_statement(R, size):
    W, H = size
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    r.copy_textures()
    worst, share = 0.0, 0.0
    for name, mean in inputs(W, H).items():
        for sigma, levels in itertools.product((0.25, 1.0), (2, 10)):
            base = Base(mean, sigma, levels, DE_LOG_ULPS)
            for (hi, lo), scale in itertools.product(((0.25, 1.0), (1.0, 0.25)), (1.0, 8.0)):
                kw = dict(highlights=hi, shadows=lo, max_ev=2.0)
                got = r.debug_local_exposure(mean, scale, sigma=sigma, levels=levels, **kw)
                ratio, s = compare(got, base, scale, kw, DE_POW2_REL, (name, sigma, levels, kw, scale))
                worst, share = max(worst, ratio), max(share, s)
    r.close()
    print("local exposure on the device %dx%d: largest |gpu - f64| / bound = %.4f, largest excluded share = %.4f" % (W, H, worst, share))
