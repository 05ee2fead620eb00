"""The leaf functions of the DE_FLAG_FAST_MATH kernel (the DE_FAST_MATH half of csrc/de_math.h, evaluated by de_debug_math_fast in the fast kernel's own
translation unit) against the float64 functions on the same float32 inputs, over the domains the path feeds them.  The bounds are composed on paper in
tests/fast_math_budget.py from what the code claims (1 ulp per hardware unit, one rounding per scaling multiply, the polynomials' stated errors) — never
from what the device returns; the figures each test prints are recorded in profiles/r5_fast_math.md."""
import numpy as np
import pytest

import fast_math_budget as fb

pytestmark = pytest.mark.gpu

FN = {"exp": 0, "log": 1, "sin": 2, "cos": 3, "atan2": 4, "asin": 5, "pow": 6, "sqrt_nr": 9, "divc": 10, "rcp_product": 11, "log_unit": 12, "rcp_nr": 13,
      "exp_nonpos": 14, "sincos_s": 15, "sincos_c": 16}


@pytest.fixture(scope="module")
def r():
    from digital_earth_amd.renderer import Renderer
    ctx = Renderer((16, 8), (0, 1, 0), texture_source="constant")
    yield ctx
    ctx.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _hold(r, name, a, b=None, what=""):
    got = r.debug_math(FN[name], a, b, fast=True)
    worst, k = fb.excess(name, got, a, b)
    rel, ab = fb.max_error(name, got, a, b)
    print("FASTLEAF %s%s: n = %d, %.3f of the budget at a = %r%s (got %r); max relative %.3e, max absolute %.3e"
          % (name, what, got.size, worst, a[k], "" if b is None else ", b = %r" % b[k], got[k], rel, ab))
    assert worst <= 1.0, (name, what, worst, a[k], None if b is None else b[k], got[k])
    return got


@pytest.mark.parametrize("name", ["exp", "exp_nonpos", "log", "sin", "cos", "sincos_s", "sincos_c", "atan2", "asin", "pow"])
def test_dense_domain_within_budget(r, name):
    a, b = fb.domain(name, np.random.default_rng(4000 + FN[name]))
    _hold(r, name, a, b)


def test_sincos_is_sin_and_cos(r):
    a, _ = fb.domain("sin", np.random.default_rng(5))
    assert (_bits(r.debug_math(15, a, fast=True)) == _bits(r.debug_math(2, a, fast=True))).all()
    assert (_bits(r.debug_math(16, a, fast=True)) == _bits(r.debug_math(3, a, fast=True))).all()


def test_log_of_every_draw(r):
    """de_log_unit on all 2^24 values k 2^-24.  log(0) = -inf: a zero draw's free flight stays +inf.  And the hook runs the fast definitions, not the
    contract's: the two differ in bits somewhere."""
    x = fb.draws()
    got = _hold(r, "log_unit", x)
    assert np.isneginf(got[0]) and np.isfinite(got[1:]).all() and (got[1:] < 0).all()
    contract = r.debug_math(12, x)
    differ = int((_bits(got) != _bits(contract)).sum())
    print("FASTLEAF log_unit: %d of 2^24 draws differ in bits from the contract's de_log_unit" % differ)
    assert differ > 0


def test_sqrt_on_every_significand(r):
    for expo in fb.SQRT_EXPONENTS:
        _hold(r, "sqrt_nr", fb.significands(expo), what=" exponent %d" % expo)


def test_reciprocal_on_every_significand(r):
    for expo in fb.RCP_EXPONENTS:
        x = fb.significands(expo)
        _hold(r, "rcp_nr", x, what=" exponent %d" % expo)
    # a quotient by a shared divisor: the numerator times the unit's reciprocal (|component| <= length ~ 6.4e6, as the contract test's real use)
    rng = np.random.default_rng(99)
    b = (6.371e6 + rng.uniform(0, 1.2e5, 1 << 22)).astype(np.float32)
    a = (rng.uniform(-1, 1, 1 << 22) * b).astype(np.float32)
    _hold(r, "rcp_product", a, b)


def test_division_by_literals(r):
    """DE_DIVC_NG(x, c) = x * RN(1 / c) for every significand of x and the literal divisors of the kernels: two roundings."""
    x = fb.significands(127)
    for c in fb.DIVISORS:
        _hold(r, "divc", x, np.full_like(x, np.float32(c)), what=" c = %r" % float(c))


def test_stated_properties(r):
    """What the comments of de_math.h state outright."""
    one = lambda fn, a, b=None: r.debug_math(fn, np.array(a, np.float32), None if b is None else np.array(b, np.float32), fast=True)
    assert np.isneginf(one(12, [0.0]))[0]                                              # de_log_unit(0) = -inf
    z = one(4, [0.0, -0.0, 0.0, -0.0], [0.0, 0.0, -0.0, -0.0])
    assert (z == 0).all()                                                              # de_atan2(0, 0) = 0
    rng = np.random.default_rng(8)
    a = np.concatenate([rng.uniform(0, 100, 4096).astype(np.float32), fb.SPECIALS])
    assert (_bits(one(6, a, np.zeros_like(a))) == _bits(np.ones_like(a))).all()        # de_pow(a, 0) = 1, for every a, NaN included
    assert (_bits(one(6, a, np.ones_like(a))) == _bits(a)).all()                       # de_pow(a, 1) = a, bit for bit
    # de_pow at a = 0 through exp2(b log2 0): 0 for b > 0, +inf for b < 0
    p = one(6, [0.0, 0.0, 0.0, 0.0], [2.5, 0.5, -0.5, -3.0])
    assert p[0] == 0 and p[1] == 0 and np.isposinf(p[2]) and np.isposinf(p[3])


def _cls(v):
    out = np.where(np.isnan(v), "nan", np.where(np.isposinf(v), "+inf", np.where(np.isneginf(v), "-inf",
          np.where(v == 0, np.where(np.signbit(v), "-0", "+0"), np.where(v > 0, "pos", "neg")))))
    return out


# Where the fast leaf returns another CLASS of value than the contract's on the special inputs (index into fb.SPECIALS), and why no loop's termination can
# depend on it.  The loops of de_stages.h end on comparisons of distances and of the free flight -log(u) / sigma; they read de_log_unit, de_sqrt_nr and
# de_rcp_nr, and everything else only shapes directions, map coordinates and weights.
_NOT_A_DRAW = "not a draw: rng_next returns k 2^-24 only, and the contract's integer reduction returns an arbitrary number there"
_RCP = ("outside the stated domain (a normal b in [2^-60, 2^60]): the contract's Newton step turns the unit's inf / 0 into NaN.  Reached only as the length of a "
        "zero vector, whose components are 0: 0 * inf = NaN either way, and the loops' NaN rules apply")
ALLOWED = {
    "exp": {8: "e^88.5 = 2.7e38 is finite; the contract saturates to +inf above 88 by definition.  de_exp feeds weights only (phase functions, Planck's law)"},
    "exp_nonpos": {4: "outside the domain (arguments <= 0 or NaN)", 8: "outside the domain (arguments <= 0 or NaN)"},
    "log": {7: "a subnormal argument is flushed by the unit: -inf for -92.1.  The fast half's de_log has no caller in the stages (de_pow uses the unit directly)"},
    "sin": {1: "sin(-0) = -0 where the contract returns +0: the two compare equal and multiply a direction component"},
    "sqrt_nr": {1: "sqrt(-0) = -0 where the contract selects +0: a length of -0 belongs to a zero vector; its reciprocal is -inf and 0 * -inf = NaN as in the contract",
                4: "outside the stated range [2^-63, 2^64]: |Q|^2 = inf needs |Q| > 1.8e19 m",
                7: "outside the stated range [2^-63, 2^64]: a subnormal |Q|^2 needs |Q| < 1e-19 m; the unit flushes it to the 0 an exact zero vector gives"},
    "log_unit": {3: _NOT_A_DRAW, 4: _NOT_A_DRAW, 5: _NOT_A_DRAW, 6: _NOT_A_DRAW, 7: _NOT_A_DRAW, 9: _NOT_A_DRAW},
    "rcp_nr": {0: _RCP, 1: _RCP, 4: _RCP, 5: _RCP, 7: _RCP},
}


@pytest.mark.parametrize("name", ["exp", "log", "sin", "cos", "atan2", "asin", "pow", "sqrt_nr", "log_unit", "rcp_nr", "exp_nonpos"])
def test_classes_on_special_values(r, name):
    """NaN, +inf, -inf, +-0 and the sign of the result on test_math_bit_exact's specials, against the contract's debug_math of the same function."""
    a = fb.SPECIALS.copy()
    b = fb.SPECIALS[::-1].copy() if name in ("atan2", "pow") else None
    if name == "atan2":     # the stated domain, as test_math_bit_exact: zero or 2^-60 <= |v| <= 2^60
        for v in (a, b):
            v[~np.isfinite(v)] = 3.0
            v[(np.abs(v) < 2.0 ** -60) & (v != 0)] = 2.0 ** -59
    fast, contract = r.debug_math(FN[name], a, b, fast=True), r.debug_math(FN[name], a, b)
    cf, cc = _cls(fast), _cls(contract)
    diff = [int(k) for k in np.nonzero(cf != cc)[0]]
    for k in diff:
        print("FASTCLASS %s(%r%s): contract %r (%s), fast %r (%s)" % (name, a[k], "" if b is None else ", %r" % b[k], contract[k], cc[k], fast[k], cf[k]))
    unlisted = [k for k in diff if k not in ALLOWED.get(name, {})]
    assert not unlisted, (name, [(float(a[k]), cc[k], cf[k]) for k in unlisted])
