"""The look LUTs of include/digital_earth_look.h restated in numpy float32, operation for operation: what look_apply_kernel must give bit for bit.
Vectorised over the pixels; every operation of the header is one line with an intermediate of its own, so that no product is ever fused with an add.
tests/test_look_ref.py holds this file to an independent float64 statement (tests/look_f64.py) and to the header's exact properties.

A table is a digital_earth_amd.cube.Cube: kind "1d" (size rows) or "3d" (size^3 rows, red fastest), with its domain."""
import numpy as np

F = np.float32
INTERPOLATIONS = ("trilinear", "tetrahedral")
DEFAULTS = dict(cube=None, shaper=None, strength=1.0, interpolation="tetrahedral", enabled=True)      # Renderer.set_look


def scale(n, lo, hi):
    """k = fl((N - 1) / (max - min)): in double from the float32 ends, rounded once."""
    return F(np.float64(n - 1) / (np.float64(F(hi)) - np.float64(F(lo))))


def coord(x, lo, hi, n):
    """(i, f) of x along one axis of a table of edge n."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = (x - F(lo)).astype(F)
        t = (d * scale(n, lo, hi)).astype(F)
        top = F(n - 1)
        t = np.where(t > F(0), np.where(t < top, t, top), F(0)).astype(F)      # NaN fails the first test
    i = np.minimum(t.astype(np.int32), np.int32(n - 2))
    f = (t - i.astype(F)).astype(F)
    return i, f


def mix(a, b, f):
    g = (F(1) - f).astype(F)
    p = (a * g).astype(F)
    q = (b * f).astype(F)
    return (p + q).astype(F)


def table_1d(x, cube):
    T = np.frombuffer(cube.table, dtype=F).reshape(cube.size, 3)
    y = np.empty_like(x)
    for c in range(3):
        i, f = coord(x[..., c], cube.domain_min[c], cube.domain_max[c], cube.size)
        y[..., c] = mix(T[i, c], T[i + 1, c], f)
    return y


def _sum4(w, v):
    """w0 v0 + w1 v1 + w2 v2 + w3 v3, the products rounded, added left to right; w: four (...,) arrays, v: four (..., 3) arrays."""
    p = [(w[k][..., None] * v[k]).astype(F) for k in range(4)]
    s = (p[0] + p[1]).astype(F)
    s = (s + p[2]).astype(F)
    return (s + p[3]).astype(F)


def table_3d(x, cube, interpolation="tetrahedral", strict=False):
    """strict=True takes, on every tie of two fractions, the OTHER neighbour's formula (`>` for `>=`): the header says the value is the same."""
    n = cube.size
    T = np.frombuffer(cube.table, dtype=F).reshape(n, n, n, 3)      # [b][g][r]
    ir, fr = coord(x[..., 0], cube.domain_min[0], cube.domain_max[0], n)
    ig, fg = coord(x[..., 1], cube.domain_min[1], cube.domain_max[1], n)
    ib, fb = coord(x[..., 2], cube.domain_min[2], cube.domain_max[2], n)

    def c(R, G, B):
        return T[ib + B, ig + G, ir + R]
    if interpolation == "trilinear":
        r, g, b = fr[..., None], fg[..., None], fb[..., None]
        c00 = mix(c(0, 0, 0), c(1, 0, 0), r)
        c10 = mix(c(0, 1, 0), c(1, 1, 0), r)
        c01 = mix(c(0, 0, 1), c(1, 0, 1), r)
        c11 = mix(c(0, 1, 1), c(1, 1, 1), r)
        c0 = mix(c00, c10, g)
        c1 = mix(c01, c11, g)
        return mix(c0, c1, b)
    if interpolation != "tetrahedral":
        raise ValueError(interpolation)
    ge = (lambda a, b: a > b) if strict else (lambda a, b: a >= b)
    one = F(1)
    sub = lambda a, b: (a - b).astype(F)      # noqa: E731
    rg, gb, rb, bg, br = ge(fr, fg), ge(fg, fb), ge(fr, fb), ge(fb, fg), ge(fb, fr)
    branches = (
        (rg & gb,         _sum4((sub(one, fr), sub(fr, fg), sub(fg, fb), fb), (c(0, 0, 0), c(1, 0, 0), c(1, 1, 0), c(1, 1, 1)))),
        (rg & ~gb & rb,   _sum4((sub(one, fr), sub(fr, fb), sub(fb, fg), fg), (c(0, 0, 0), c(1, 0, 0), c(1, 0, 1), c(1, 1, 1)))),
        (rg & ~gb & ~rb,  _sum4((sub(one, fb), sub(fb, fr), sub(fr, fg), fg), (c(0, 0, 0), c(0, 0, 1), c(1, 0, 1), c(1, 1, 1)))),
        (~rg & bg,        _sum4((sub(one, fb), sub(fb, fg), sub(fg, fr), fr), (c(0, 0, 0), c(0, 0, 1), c(0, 1, 1), c(1, 1, 1)))),
        (~rg & ~bg & br,  _sum4((sub(one, fg), sub(fg, fb), sub(fb, fr), fr), (c(0, 0, 0), c(0, 1, 0), c(0, 1, 1), c(1, 1, 1)))),
        (~rg & ~bg & ~br, _sum4((sub(one, fg), sub(fg, fr), sub(fr, fb), fb), (c(0, 0, 0), c(0, 1, 0), c(1, 1, 0), c(1, 1, 1)))),
    )
    y = np.zeros(x.shape, F)
    seen = np.zeros(x.shape[:-1], bool)
    for mask, value in branches:
        assert not (mask & seen).any()
        seen |= mask
        y[mask] = value[mask]
    assert seen.all()
    return y


def apply(x, cube=None, shaper=None, strength=1.0, interpolation="tetrahedral", strict=False):
    """The stage on (..., 3) float32 pixels: the 1D table, the 3D table on its result, the mix with the original, the clamp."""
    shape = np.shape(x)
    x = np.ascontiguousarray(x, dtype=F).reshape(-1, 3)
    assert cube is not None or shaper is not None
    y = x
    if shaper is not None:
        assert shaper.kind == "1d"
        y = table_1d(y, shaper)
    if cube is not None:
        assert cube.kind == "3d"
        y = table_3d(y, cube, interpolation, strict)
    s = F(strength)
    keep = F(F(1) - s)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (x * keep).astype(F)
        q = (y * s).astype(F)
        o = (p + q).astype(F)
        return np.where(o > F(0), np.where(o < F(1), o, F(1)), F(0)).astype(F).reshape(shape)
