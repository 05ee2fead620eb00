"""Error budgets of the DE_FAST_MATH half of csrc/de_math.h, composed on paper from what the code claims, and a float64 restatement of its formulas.

Nothing here is measured from the device.  The inputs of every composition are:
  ULP = 2^-23   one unit in the last place, relative: what de_math.h claims for the result of v_exp_f32, v_log_f32, v_sqrt_f32 and v_rcp_f32
  SINCOS_ABS = 2^-22, SINCOS_REL = 2^-20   what it claims for v_sin_f32 / v_cos_f32: the smaller of an absolute and a relative error (the header said "1 ulp"
                like the others until this test disproved it; DESIGN.md §2 has the corrected claim and why the path tolerates it)
  U   = 2^-24   one float32 rounding to nearest, relative: every scaling multiply and every fma of a polynomial
  the error of each float32 constant against the real number it stands for (computed below from the constants, copied as data)
  the polynomials' stated errors: 1.73e-5 rad for the four-coefficient atan2, 1.9e-7 rad for the contract's asin polynomial
  TINY = 2^-126  a hardware unit may flush a subnormal result to zero

budget(name, a, b) returns (rel, abs): the device must meet |got - f| <= rel * |f| + abs against the float64 function f on the same float32 inputs.
exact_part(name, a, b) is the same bound without any float32 rounding and without the units' ulps: what the float64 restatement (restate) of the same
formulas must meet with exact units.  tests/test_fast_math_budget.py holds the restatement to it, which pins the coefficients and constants without a
device, and shows that three seeded faults exceed it."""
import numpy as np

ULP = 2.0 ** -23
U = 2.0 ** -24
TINY = 2.0 ** -126
SINCOS_ABS = 2.0 ** -22
SINCOS_REL = 2.0 ** -20

# the constants and coefficients of the DE_FAST_MATH half, copied as data (C99 hex floats, exact in float32)
CONSTS = {
    "PI": float.fromhex("0x1.921fb6p+1"),
    "PIO2": float.fromhex("0x1.921fb6p+0"),
    "LOG2E": float.fromhex("0x1.715476p+0"),
    "LN2": float.fromhex("0x1.62e430p-1"),
    "INV_2PI": float(np.float32(0.5 / np.pi)),
    "INV_PI": float(np.float32(1.0 / np.pi)),
    "ATAN": tuple(float.fromhex(h) for h in ("0x1.79d11ep-6", "-0x1.727c04p-4", "0x1.79d652p-3", "-0x1.53a54cp-2")),      # highest power first
    "ASIN": tuple(float.fromhex(h) for h in ("0x1.a7813ap-5", "0x1.409a72p-5", "0x1.35737ap-4", "0x1.554bf8p-3")),
}
E_LOG2E = abs(CONSTS["LOG2E"] * np.log(2.0) - 1.0)          # relative error of each constant: 1.3e-8, 2.7e-9, 2.0e-8, 2.8e-8, 2.8e-8
E_LN2 = abs(CONSTS["LN2"] / np.log(2.0) - 1.0)
E_INV_2PI = abs(CONSTS["INV_2PI"] * 2.0 * np.pi - 1.0)
E_PI = abs(CONSTS["PI"] - np.pi)                             # absolute: 8.7e-8, 4.4e-8
E_PIO2 = abs(CONSTS["PIO2"] - np.pi / 2)
ATAN_POLY = 1.73e-5      # rad: the four-coefficient fit on [0, 1] (de_math.h; its maximum in exact arithmetic is 1.7216e-5)
ASIN_POLY = 1.9e-7       # rad: the contract's four-coefficient asin, as DESIGN.md §2 states it (its maximum in exact arithmetic is 6.0e-8)

# the literal divisors of DE_DIVC_NG (tests/test_gpu_parity.py::test_three_operation_division_by_literals)
DIVISORS = (255.0, np.float32(np.pi), 49.0, np.float32(532307548.4168), np.float32(1.225), np.float32(8136.646), 6000.0,
            np.float32(0.1) * np.float32(0.029), np.float32(0.02) * np.float32(0.029))


def compose(*rels):
    """(1 + r1)(1 + r2) ... - 1: relative errors of successive factors."""
    out = 1.0
    for r in rels:
        out = out * (1.0 + r)
    return out - 1.0


def _f64(v):
    return None if v is None else np.asarray(v, np.float32).astype(np.float64)


def reference(name, a, b=None):
    """The float64 function of the float32 inputs."""
    a, b = _f64(a), _f64(b)
    with np.errstate(all="ignore"):
        if name in ("exp", "exp_nonpos"): return np.exp(a)
        if name in ("log", "log_unit"): return np.log(a)
        if name in ("sin", "sincos_s"): return np.sin(a)
        if name in ("cos", "sincos_c"): return np.cos(a)
        if name == "atan2": return np.where((a == 0) & (b == 0), 0.0, np.arctan2(a + 0.0, b))      # de_atan2(0, 0) = 0 by definition; y = -0 counts as +0 (the code tests y < 0)
        if name == "asin": return np.arcsin(np.clip(a, -1.0, 1.0))
        if name == "pow": return np.where(b == 0, 1.0, np.power(a, b))
        if name == "sqrt_nr": return np.sqrt(a)
        if name == "rcp_nr": return 1.0 / a
        if name in ("divc", "rcp_product"): return a / b
    raise KeyError(name)


def restate(name, a, b=None, consts=CONSTS):
    """The formulas of the DE_FAST_MATH half in float64, with exact units (exp2, log2, sin, cos of revolutions, sqrt, reciprocal) and the float32 constants
    and coefficients of `consts`.  What remains against reference() is the polynomials' and the constants' error."""
    a, b = _f64(a), _f64(b)
    c = consts
    with np.errstate(all="ignore"):
        if name in ("exp", "exp_nonpos"): return np.exp2(a * c["LOG2E"])
        if name in ("log", "log_unit"): return np.log2(a) * c["LN2"]
        if name in ("sin", "sincos_s"): return np.sin(2.0 * np.pi * (a * c["INV_2PI"]))
        if name in ("cos", "sincos_c"): return np.cos(2.0 * np.pi * (a * c["INV_2PI"]))
        if name == "atan2":
            y, x = a, b
            ax, ay = np.abs(x), np.abs(y)
            swap = ay > ax
            mx, mn = np.where(swap, ay, ax), np.where(swap, ax, ay)
            q = mn * (1.0 / mx)
            s = q * q
            p = c["ATAN"][0]
            for k in c["ATAN"][1:]:
                p = p * s + k
            r = q * s * p + q
            r = np.where(swap, c["PIO2"] - r, r)
            r = np.where(x < 0, c["PI"] - r, r)
            r = np.where(y < 0, -r, r)
            return np.where(mx == 0, 0.0, r)
        if name == "asin":
            ax = np.minimum(np.abs(a), 1.0)
            big = ax > 0.5
            s = np.where(big, (1.0 - ax) * 0.5, ax * ax)
            t = np.where(big, np.sqrt(s), ax)
            p = c["ASIN"][0]
            for k in c["ASIN"][1:]:
                p = p * s + k
            r = t * s * p + t
            r = np.where(big, c["PIO2"] - 2.0 * r, r)
            return np.where(a < 0, -r, r)
        if name == "pow": return np.where(b == 0, 1.0, np.where(b == 1, a, np.exp2(b * np.log2(a))))
        if name == "sqrt_nr": return np.sqrt(a)
        if name == "rcp_nr": return 1.0 / a
        if name == "divc": return a * (1.0 / b)
        if name == "rcp_product": return a * (1.0 / b)
    raise KeyError(name)


def exact_part(name, a, b=None):
    """(rel, abs) the float64 restatement must meet: constants and polynomials only."""
    a, b = _f64(a), _f64(b)
    if name in ("exp", "exp_nonpos"):
        # the argument x * LOG2E carries the constant's relative error: 2^(x log2e (1 + e)) = e^x * e^(x e)
        return np.expm1(np.abs(a) * E_LOG2E), 0.0
    if name in ("log", "log_unit"):
        return E_LN2, 0.0
    if name in ("sin", "cos", "sincos_s", "sincos_c"):
        # the angle x * INV_2PI * 2 pi is off by |x| e; |d sin| <= |d angle|
        return 0.0, np.abs(a) * E_INV_2PI
    if name == "atan2":
        return 0.0, ATAN_POLY + E_PI          # the fit, and the constant the reflections subtract from (PI; PIO2's error is half of it)
    if name == "asin":
        return 0.0, ASIN_POLY + E_PIO2
    if name in ("pow", "sqrt_nr", "rcp_nr", "divc", "rcp_product"):
        return 0.0, 0.0                       # exact formulas: only float64's own rounding remains (the test allows 1e-13 relative)
    raise KeyError(name)


def budget(name, a, b=None):
    """(rel, abs) for the device.  Each derivation in a few lines."""
    a, b = _f64(a), _f64(b)
    if name in ("exp", "exp_nonpos"):
        # y = RN(x * LOG2E): relative error U + E_LOG2E in the argument, i.e. a factor e^(|x| (U + e)) on the result ("|x| 2^-24 relative through the
        # argument"); v_exp_f32: 1 ulp.  A result below 2^-126 may be flushed (the contract's de_exp returns 0 below e^-87 itself).
        return compose(ULP, np.expm1(np.abs(a) * (U + E_LOG2E))), TINY
    if name in ("log", "log_unit"):
        # v_log_f32: 1 ulp of log2 x; the product with LN2: one rounding and the constant's error
        return compose(ULP, U, E_LN2), 0.0
    if name in ("sin", "cos", "sincos_s", "sincos_c"):
        # r = RN(x * INV_2PI) revolutions: the angle is off by |x| (U + e) rad, and |d sin| <= |d angle|; v_sin_f32 / v_cos_f32: min(2^-20 |f|, 2^-22)
        return 0.0, np.minimum(SINCOS_REL * np.abs(reference(name, a)), SINCOS_ABS) + np.abs(a) * (U + E_INV_2PI)
    if name == "atan2":
        # q = mn * rcp(mx): relative ULP + U, and q / (1 + q^2) <= 1/2: 0.75 * 2^-23 rad;  s, three fmas of p (|p| < 1/3 on |q s| <= 1), q s and the last fma:
        # under 4 U;  PIO2 - r: U (half an ulp below 2) + E_PIO2;  PI - r: 2 U (half an ulp below 4) + E_PI.  Sum < 1.5 U + 4 U + U + 2 U + E_PIO2 + E_PI
        # = 8.5 U + 1.3e-7 < 11 U.  Added to the fit's 1.73e-5 rad.
        return 0.0, ATAN_POLY + 11.0 * U
    if name == "asin":
        # big branch: t = sqrt(s) (1 + ULP) with t <= 1/2, doubled by the reflection: 2^-23 rad;  roundings of t s, the fma (r < 0.79) and the reflection's
        # fma (result < 2): under 3 U;  E_PIO2 = 0.73 U.  Small branch: the same roundings without the root.  Added to the polynomial's 1.9e-7 rad.
        return 0.0, ASIN_POLY + ULP + 4.0 * U
    if name == "pow":
        # exp2(RN(b * log2 a)): the exponent e = b log2 a is off by |e| (ULP + U) (v_log_f32's ulp and the product's rounding), a factor 2^(|e| (ULP + U)) on
        # the result; v_exp_f32: 1 ulp.  b = 0 and b = 1 return 1 and a exactly.
        with np.errstate(all="ignore"):
            e = np.abs(b * np.log2(a))
        e = np.where(np.isfinite(e) & (b != 0) & (b != 1), e, 0.0)
        return np.where((b == 0) | (b == 1), 0.0, compose(ULP, np.expm1(np.log(2.0) * e * (ULP + U)))), TINY
    if name in ("sqrt_nr", "rcp_nr"):
        return ULP, 0.0                       # the unit's result as it is
    if name == "divc":
        return compose(U, U), 0.0             # x * RN(1 / c): two roundings
    if name == "rcp_product":
        return compose(ULP, U), 0.0           # x * v_rcp_f32(y): the unit's ulp and one rounding
    raise KeyError(name)


def excess(name, got, a, b=None, bound=budget):
    """max over the inputs of |got - f| / (rel |f| + abs) (<= 1: within the bound), and the index where.  Where f is infinite, NaN or exactly zero with a zero
    bound, got must be the same value and counts as 0, else as inf."""
    f = reference(name, a, b)
    got = np.asarray(got).astype(np.float64)
    rel, ab = bound(name, a, b)
    with np.errstate(all="ignore"):
        tol = rel * np.abs(f) + ab
        err = np.abs(got - f)
        ratio = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    special = ~np.isfinite(f)
    same = (np.isnan(f) & np.isnan(got)) | (f == got)
    ratio = np.where(special, np.where(same, 0.0, np.inf), ratio)
    k = int(np.argmax(ratio))
    return float(ratio[k]), k


def max_error(name, got, a, b=None):
    """The measured maxima for the record: (max relative error where |f| > 0 and finite, max absolute error)."""
    f = reference(name, a, b)
    got = np.asarray(got).astype(np.float64)
    ok = np.isfinite(f) & np.isfinite(got)
    err = np.abs(got - f)[ok]
    with np.errstate(all="ignore"):
        rel = np.where(f[ok] != 0, err / np.abs(f[ok]), 0.0)
    return float(rel.max()) if rel.size else 0.0, float(err.max()) if err.size else 0.0


# ---- the input generators (the domains the path feeds each function; the dense ones are those of tests/test_gpu_parity.py)
def significands(expo):
    return ((np.uint32(expo) << np.uint32(23)) | np.arange(1 << 23, dtype=np.uint32)).view(np.float32)


SQRT_EXPONENTS = (127, 128, 172, 173, 97, 110, 111, 64, 65, 190, 191)      # test_fast_sqrt_is_correctly_rounded
RCP_EXPONENTS = (127, 126, 149, 150, 100, 180)                             # test_fast_reciprocal_is_correctly_rounded
SPECIALS = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-40, 88.5, -87.5, 0.5, 2.0 ** -24], np.float32)      # test_math_bit_exact


def draws():
    """Every value rng_next can return: k * 2^-24."""
    return (np.arange(1 << 24, dtype=np.float64) * 2.0 ** -24).astype(np.float32)


def unit_vector_components(n, rng):
    """(y, x) pairs as sphere_UV_map forms them: two components of unit vectors, with the axes, the swap boundary |y| = |x| and its neighbours."""
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    y, x = v[:, 2].astype(np.float32), (-v[:, 0]).astype(np.float32)
    h = np.float32(np.sqrt(0.5))
    edge = []
    for sy in (1.0, -1.0):
        for sx in (1.0, -1.0):
            edge += [(sy * h, sx * h), (sy * np.nextafter(h, np.float32(1)), sx * h), (sy * h, sx * np.nextafter(h, np.float32(1))),
                     (sy * 0.25, sx * 0.25), (sy * 1e-3, sx * 1e-3), (sy * 2.0 ** -30, sx * 1.0), (sy * 1.0, sx * 2.0 ** -30)]
    edge += [(0.0, 1.0), (0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (-0.0, 1.0), (-0.0, -1.0), (1.0, -0.0), (0.0, 0.0), (0.0, 0.5), (0.5, 0.0)]
    e = np.array(edge, np.float32)
    y[:len(e)], x[:len(e)] = e[:, 0], e[:, 1]
    # the whole swap boundary, densely: |y| = |x| exactly, all four quadrants
    m = min(n // 4, 1 << 16)
    d = rng.uniform(2.0 ** -20, 1.0, m).astype(np.float32)
    sl = slice(len(e), len(e) + m)
    y[sl], x[sl] = d * np.sign(rng.standard_normal(m)).astype(np.float32), d * np.sign(rng.standard_normal(m)).astype(np.float32)
    return y, x


def domain(name, rng, n=1 << 20):
    """Dense inputs (a, b) of each function."""
    if name == "exp":          # test_math_bit_exact's range cut at the issue's ends: down to underflow, up to 88.5
        x = rng.uniform(-104.0, 88.5, n).astype(np.float32)
        x[:6] = [0.0, -0.0, 88.5, -87.0, -87.3365, 1.0]
        return x, None
    if name == "exp_nonpos":   # test_exp_of_a_non_positive_argument
        x = np.concatenate([-np.abs(rng.standard_normal(n)).astype(np.float32) * np.float32(40.0), -np.linspace(0.0, 104.0, n // 4, dtype=np.float32),
                            np.array([0.0, -0.0, -87.0, -87.00001, -1e-30], np.float32)])
        return x, None
    if name == "log":
        return np.exp(rng.uniform(-85, 85, n)).astype(np.float32), None
    if name in ("sin", "cos", "sincos_s", "sincos_c"):
        # the angles the path forms: 2 pi u for every kind of draw u (dense, and the smallest and largest), the sun's cone angle; and +-20 as the contract test
        u = rng.integers(0, 1 << 24, n // 2).astype(np.float64) * 2.0 ** -24
        phi = (np.float32(2.0 * np.pi) * u.astype(np.float32)).astype(np.float32)
        k = np.array([0, 1, 2, 3, (1 << 22), (1 << 23), 3 << 22, (1 << 24) - 1, (1 << 23) + 1, (1 << 23) - 1], np.float64) * 2.0 ** -24
        x = np.concatenate([phi, (np.float32(2.0 * np.pi) * k.astype(np.float32)).astype(np.float32), np.array([0.0, -0.0, 0.00465, 20.0, -20.0], np.float32),
                            rng.uniform(-20, 20, n // 2).astype(np.float32)])
        return x, None
    if name == "atan2":
        return unit_vector_components(n, rng)
    if name == "asin":
        x = rng.uniform(-1.001, 1.001, n).astype(np.float32)
        e = np.array([0.0, -0.0, 0.5, -0.5, 1.0, -1.0, np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(1), np.float32(0)), 1.001, -1.001, 1e-20], np.float32)
        x[:len(e)] = e
        return x, None
    if name == "pow":
        a, b = rng.uniform(0, 100, n).astype(np.float32), rng.uniform(-3, 3, n).astype(np.float32)
        a[:4] = [0.0, 0.0, 1.0, 100.0]; b[:4] = [2.5, 0.5, -3.0, 3.0]
        return a, b
    raise KeyError(name)
