"""The DE_FAST_MATH half of csrc/de_math.h without a device: its coefficients and constants, copied as data into tests/fast_math_budget.py, evaluated in
float64 with exact units, meet the polynomial and constant parts of the error budgets the GPU test (tests/test_gpu_fast_math_leaves.py) holds the device to;
the copies are the header's; and three seeded faults show the check can fail."""
import os
import re

import numpy as np
import pytest

import fast_math_budget as fb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("exp", "exp_nonpos", "log", "sin", "cos", "atan2", "asin", "pow")


def _inputs(name):
    return fb.domain(name, np.random.default_rng(77), 1 << 18)


def _excess(name, a, b, consts=fb.CONSTS, bound=fb.exact_part):
    # float64's own roundings (a few 1e-16 per operation, amplified by |x| log2e <= 150 in exp and by 3 log2(100) in pow): 1e-13 relative, 1e-15 absolute
    def with_f64_slack(nm, aa, bb):
        rel, ab = bound(nm, aa, bb)
        return rel + 1e-13, ab + 1e-15
    return fb.excess(name, fb.restate(name, a, b, consts), a, b, bound=with_f64_slack)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_meets_the_exact_part_of_the_budget(name):
    a, b = _inputs(name)
    worst, k = _excess(name, a, b)
    print("%s: %.3f of the exact part at a = %r" % (name, worst, a[k]))
    assert worst <= 1.0, (name, worst, a[k], None if b is None else b[k])
    # and the exact part is inside the device's budget everywhere
    (r0, a0), (r1, a1) = fb.exact_part(name, a, b), fb.budget(name, a, b)
    assert np.all(r0 <= r1) and np.all(a0 <= a1)


def test_log_of_every_draw_in_float64():
    x = fb.draws()
    worst, k = _excess("log_unit", x, None)
    assert worst <= 1.0, (worst, x[k])
    assert np.isneginf(fb.restate("log_unit", x[:1])[0])


def test_polynomial_claims():
    """The figures de_math.h states.  The four-coefficient atan2 reaches 1.7216e-5 rad in exact arithmetic — above the 1.7e-5 the header used to state, below
    the 1.73e-5 it states now; that is 0.0592 texel of a 21 600-wide map, so "0.06 texel" stands.  The asin polynomial with an exact root stays inside 1.9e-7."""
    q = np.linspace(0.0, 1.0, 2_000_001).astype(np.float32)
    one = np.ones_like(q)
    err = np.abs(fb.restate("atan2", q, one) - np.arctan(q.astype(np.float64))).max()
    print("atan2 fit: %.4e rad = %.4f texel" % (err, err / (2 * np.pi / 21600)))
    assert 1.70e-5 < err <= fb.ATAN_POLY
    assert fb.ATAN_POLY / (2 * np.pi / 21600) < 0.06
    x = np.linspace(-1.0, 1.0, 2_000_001).astype(np.float32)
    assert np.abs(fb.restate("asin", x) - np.arcsin(x.astype(np.float64))).max() <= fb.ASIN_POLY


def test_copied_constants_are_the_headers():
    text = open(os.path.join(ROOT, "digital_earth_amd", "csrc", "de_math.h")).read()
    fast = text[text.index("#ifdef DE_FAST_MATH"):text.index("#else")]
    for name in ("PI", "PIO2", "LOG2E", "LN2"):
        m = re.search(r"#define DE_%s (\S+?)f\s" % name, fast)
        assert float.fromhex(m.group(1)) == fb.CONSTS[name], name
    assert "#define DE_INV_2PI ((float)(0.5 / 3.14159265358979323846))" in fast
    for fn, key in (("de_atan2", "ATAN"), ("de_asin", "ASIN")):
        body = fast[fast.index("DE_DEV float %s(" % fn):]
        body = body[:body.index("\n}")]
        hexes = [float.fromhex(h) for h in re.findall(r"(-?0x1\.[0-9a-f]+p[+-]\d+)f", body)]
        assert tuple(hexes[:4]) == fb.CONSTS[key], fn
    assert "1.73e-5 rad" in fast and "1.7e-5 rad" not in fast


def _fault(**kw):
    return dict(fb.CONSTS, **kw)


def test_seeded_faults_exceed_the_budget():
    """Each fault is applied to the float64 restatement; the figure is the miss as a multiple of the bound.
    (a) the last atan2 coefficient -0x1.53a54cp-2 with its last hex digit changed to 0: 1.7395e-5 rad.  A change of a last hex digit moves the fit by at most
        1.8e-7 rad, less than the 6.6e-7 rad the device's budget allows for float32 roundings, so this one is caught by the exact part only (the CPU check above),
        not on the device.
    (b) DE_INV_2PI replaced by DE_INV_PI: sin(2x) for sin(x).
    (c) DE_LN2 truncated to 0x1.62e4p-1: 2.06e-6 relative.
    (b) and (c) exceed the device's whole budget too."""
    y, x = _inputs("atan2")
    atan = list(fb.CONSTS["ATAN"]); atan[3] = float.fromhex("-0x1.53a540p-2")
    worst, _ = _excess("atan2", y, x, _fault(ATAN=tuple(atan)))
    print("atan2 coefficient: %.4f of the exact part" % worst)
    assert worst > 1.0
    for name in ("sin", "cos"):
        a, _b = _inputs(name)
        for bound in (fb.exact_part, fb.budget):
            worst, _ = _excess(name, a, None, _fault(INV_2PI=fb.CONSTS["INV_PI"]), bound)
            assert worst > 1e4, (name, worst)
    for name, a in (("log", _inputs("log")[0]), ("log_unit", fb.draws()[1::257])):
        for bound in (fb.exact_part, fb.budget):
            worst, _ = _excess(name, a, None, _fault(LN2=float.fromhex("0x1.62e4p-1")), bound)
            print("%s with the truncated LN2: %.2f of %s" % (name, worst, bound.__name__))
            assert worst > 1.0, (name, worst)
