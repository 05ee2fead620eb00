"""The panorama stage (include/digital_earth_panorama.h) restated twice, for the tests.

1. `panorama(...)`: the kernel's arithmetic in numpy float32, operation by operation as the header defines it (no fused operation: every numpy
   float32 operation rounds on its own).  Its two leaves are injectable: `sincos(theta) -> (sin, cos)` and `sqrt(x)`, float32 arrays in and out.
   The defaults are numpy's correctly rounded square root and a port of de_math.h's de_sincos whose fused multiply-adds are evaluated exactly; the
   GPU tests hand in the device's own values (Renderer.debug_math functions 2, 3 and 8) instead.
2. `f64_*`: an independent float64 statement of the GEOMETRY alone — the direction of an output position, the face cameras of the header's table,
   and the renderer's cast through such a camera (get_cast_dir's formula, the jitter replaced by the fractional position, its 1e-5 offset dropped as
   the stage's header drops it).  It shares no code with 1.
3. `f64_linear_*`: an independent float64 statement of the IMAGE: six faces filled with a field that is linear on every face, built from 2. alone,
   and the closed form of what any correct resampling of them holds at a direction.  It knows of no tap, no face index and no table.
"""
import numpy as np

F = np.float32
PROJECTIONS = ("equirect", "fisheye")
DEFAULTS = dict(size=None, projection="equirect", aperture=180.0, apron=1, supersample=2, basis=None, on=True)
STRUCT_BYTES = 68
# face 0 ... 5 = +r, -r, +u, -u, +f, -f: (row of the basis, sign) of its look and of its up
LOOK = ((0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1))
UP = ((1, 1), (1, 1), (2, -1), (2, 1), (1, 1), (1, 1))
TILE, MAX_S = 32, 4            # panorama_body.h's PANO_TILE and PANO_MAX_S: one workgroup's square of the output, the largest supersample
# Outputs of more than one tile along the second axis (tests/test_panorama_ref.py states in numpy what each is there for; the GPU tests run them):
MULTI_TILE = [((96, 40), "equirect", 180.0),      # 3 x 2 tiles: a swapped / and % in the tile decode lands elsewhere; the last tile row has 8 rows
              ((48, 72), "equirect", 180.0),      # 2 x 3 tiles, partial on both axes (16 columns, 8 rows)
              ((48, 48), "fisheye", 90.0),        # 2 x 2 tiles, partial on both axes; every sample on +f or one of its four neighbours
              ((80, 80), "fisheye", 220.0)]       # 3 x 3 tiles, partial; directions behind the equator of the frame
# Face sizes and aprons of those runs: de_create's smallest square with the smallest and the largest apron, and one N that is no power of two and exceeds
# a tile (its face rows have a 120-float stride)
FACE_SIZES = ((16, 1), (16, 4), (40, 10))
# The float32 restatement of f64_linear_faces against f64_linear_image, the largest absolute error over every case of tests/test_panorama_ref.py's
# linear-field test (values reach about 2): measured on the restatement alone with numpy's leaves, per supersample.  The bound of that test and of the
# GPU's is FOUR times this: the device's de_sincos may differ from the port's by an ulp in the fisheye.  A half-pixel or a transposition is an error of
# about fov / N = 0.07 at N = 16, five orders above.
LINEAR_MEASURED = {1: 5.7e-7, 4: 4.1e-7}      # 5.64e-7 (80 x 80 fisheye at 220°, apron 1) and 4.05e-7 (32 x 32 fisheye at 360°, apron 1), rounded up
LINEAR_BOUND = {S: 4.0 * m for S, m in LINEAR_MEASURED.items()}      # 2.28e-6 and 1.64e-6


# ---------------------------------------------------------------- the leaves
def fma(a, b, c):
    """round32(a b + c) for float32 arrays, exactly: the product is exact in float64; the sum's float64 rounding error (TwoSum) decides the one
    case in which rounding twice differs from rounding once, a float64 sum that lies exactly half-way between two float32 values."""
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    p = a * b
    t = p + c
    bp = t - p
    e = (p - (t - bp)) + (c - bp)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = np.nextafter(t, np.inf).astype(F)
        lo = np.nextafter(t, -np.inf).astype(F)
        mid = (hi != lo) & ((hi.astype(np.float64) - t) == (t - lo.astype(np.float64)))
        r = t.astype(F)
    return np.where(mid & (e > 0), hi, np.where(mid & (e < 0), lo, r)).astype(F)


def H(text):
    return F(float.fromhex(text))


def de_sincos(x):
    """de_math.h's de_sincos (the arithmetic contract's half), float32 in, (sin, cos) float32 out."""
    x = np.asarray(x, F)
    k = np.floor(fma(x, H("0x1.45f306p-1"), F(0.5)))
    r = fma(-k, H("0x1.92p+0"), x)
    r = fma(-k, H("0x1.fb4p-12"), r)
    r = fma(-k, H("0x1.4442d2p-24"), r)
    q = k.astype(np.int64) & 3
    r2 = r * r
    ps = np.full_like(r, H("0x1.6cca94p-19"))
    ps = fma(ps, r2, H("-0x1.a00f5ap-13"))
    ps = fma(ps, r2, H("0x1.111108p-7"))
    ps = fma(ps, r2, H("-0x1.555556p-3"))
    sn = fma(r * r2, ps, r)
    pc = np.full_like(r, H("-0x1.241daap-22"))
    pc = fma(pc, r2, H("0x1.a010dap-16"))
    pc = fma(pc, r2, H("-0x1.6c16b8p-10"))
    pc = fma(pc, r2, H("0x1.555556p-5"))
    cs = fma(r2 * r2, pc, fma(F(-0.5), r2, F(1.0)))
    s = np.where(q & 1, cs, sn)
    c = np.where(q & 1, sn, cs)
    s = np.where(q & 2, -s, s)
    c = np.where((q + 1) & 2, -c, c)
    return s.astype(F), c.astype(F)


def de_sqrt(x):
    return np.sqrt(np.asarray(x, F))


# ---------------------------------------------------------------- 1. the restatement
def _basis(basis):
    return np.asarray(np.eye(3) if basis is None else basis, dtype=F).reshape(3, 3)


def consts(N, apron=1, aperture=180.0, basis=None):
    """What the library computes once per de_set_panorama, in double from the float32 settings, rounded once: fov, scale, half_aperture, m[6][4]."""
    B = _basis(basis).astype(np.float64)
    fov = F(float(N) / float(N - 2 * apron))
    scale = F(float(N) / (2.0 * float(fov)))
    half = F(float(F(aperture)) * 3.14159265358979323846 / 360.0)
    m = np.zeros((6, 4), F)
    for face in range(6):
        d = LOOK[face][1] * B[LOOK[face][0]]
        up = UP[face][1] * B[UP[face][0]]
        du = np.cross(d, up)
        du = du / np.sqrt((du * du).sum())
        dv = np.cross(du, d)
        dv = dv / np.sqrt((dv * dv).sum())
        axis = face // 2
        e1, e2 = B[1 if axis == 0 else 0], B[1 if axis == 2 else 2]
        m[face] = [F(_dot(e1, du)), F(_dot(e2, du)), F(_dot(e1, dv)), F(_dot(e2, dv))]
    return fov, scale, half, m


def _dot(a, b):
    s = 0.0
    for k in range(3):
        s += a[k] * b[k]
    return s


def tables(n, S, span):
    """sin and cos of entry k of an axis of n S entries: the angle ((k + 0.5) / (n S) - 0.5) span, in double, rounded once."""
    m = n * S
    ang = ((np.arange(m, dtype=np.float64) + 0.5) / float(m) - 0.5) * span
    return np.sin(ang).astype(F), np.cos(ang).astype(F)


def locate(cr, cu, cf, N, k):
    """Components along r, u, f (float32 arrays) -> (face, X, Y): the face and the unclamped pixel coordinates in it."""
    fov, scale, _, m = k
    cr, cu, cf = (np.asarray(v, F) for v in (cr, cu, cf))
    ar, au, af = np.abs(cr), np.abs(cu), np.abs(cf)
    is_r = (ar >= au) & (ar >= af)
    is_u = ~is_r & (au >= af)
    with np.errstate(divide="ignore", invalid="ignore"):
        face = np.where(is_r, np.where(cr < 0, 1, 0), np.where(is_u, np.where(cu < 0, 3, 2), np.where(cf < 0, 5, 4)))
        mag = np.where(is_r, ar, np.where(is_u, au, af))
        p = np.where(is_r, cu, cr) / mag
        q = np.where(is_r | is_u, cf, cu) / mag
        mm = m[face]
        fu = p * mm[..., 0] + q * mm[..., 1]
        fv = p * mm[..., 2] + q * mm[..., 3]
        X = (fu + fov) * scale - F(0.5)
        Y = (fv + fov) * scale - F(0.5)
    return face, X.astype(F), Y.astype(F)


def _sample(faces, cr, cu, cf, N, k):
    face, X, Y = locate(cr, cu, cf, N, k)
    top = F(N - 1)
    with np.errstate(invalid="ignore"):
        X = np.where(X > 0, np.where(X < top, X, top), F(0)).astype(F)
        Y = np.where(Y > 0, np.where(Y < top, Y, top), F(0)).astype(F)
    i0 = np.minimum(np.floor(X).astype(np.int64), N - 2)
    j0 = np.minimum(np.floor(Y).astype(np.int64), N - 2)
    ax = (X - i0.astype(F))[..., None]
    ay = (Y - j0.astype(F))[..., None]
    c00, c10 = faces[face, i0, j0], faces[face, i0 + 1, j0]
    c01, c11 = faces[face, i0, j0 + 1], faces[face, i0 + 1, j0 + 1]
    with np.errstate(invalid="ignore", over="ignore"):
        t0 = c00 + ax * (c10 - c00)
        t1 = c01 + ax * (c11 - c01)
        return (t0 + ay * (t1 - t0)).astype(F)


def sub_direction(size, projection, S, a, b, k, sincos=None, sqrt=None, tabs=None):
    """Sub-position (a, b) of every output pixel -> (cr, cu, cf, outside), arrays (width, height); outside: beyond the fisheye's circle."""
    w, h = size
    sincos, sqrt = sincos or de_sincos, sqrt or de_sqrt
    ki = (np.arange(w) * S + a)[:, None] + np.zeros((1, h), np.int64)
    kj = (np.arange(h) * S + b)[None, :] + np.zeros((w, 1), np.int64)
    if projection == "equirect":
        (sl, cl), (st, ct) = tabs or (tables(w, S, 2.0 * np.pi), tables(h, S, np.pi))
        return ct[kj] * sl[ki], st[kj] + np.zeros_like(sl[ki]), ct[kj] * cl[ki], np.zeros((w, h), bool)
    px = (2 * ki + 1).astype(F) / F(w * S) - F(1)
    py = (2 * kj + 1).astype(F) / F(h * S) - F(1)
    rho = sqrt((px * px + py * py).astype(F).ravel()).reshape(w, h)
    sn, cs = sincos((rho * k[2]).astype(F).ravel())
    sn, cs = sn.reshape(w, h), cs.reshape(w, h)
    with np.errstate(divide="ignore", invalid="ignore"):
        cr, cu, cf = sn * (px / rho), sn * (py / rho), cs
    zero = rho == 0
    return np.where(zero, F(0), cr).astype(F), np.where(zero, F(0), cu).astype(F), np.where(zero, F(1), cf).astype(F), rho > 1


def panorama(faces, size, projection="equirect", aperture=180.0, apron=1, supersample=2, basis=None, sincos=None, sqrt=None):
    """faces (6, N, N, 3) float32 -> (width, height, 3) float32, as panorama_kernel computes it."""
    faces = np.ascontiguousarray(faces, F)
    N, S, (w, h) = faces.shape[1], int(supersample), size
    k = consts(N, apron, aperture, basis)
    tabs = (tables(w, S, 2.0 * np.pi), tables(h, S, np.pi)) if projection == "equirect" else None
    mean, n = None, 0
    for b in range(S):
        for a in range(S):
            cr, cu, cf, outside = sub_direction(size, projection, S, a, b, k, sincos, sqrt, tabs)
            v = _sample(faces, cr, cu, cf, N, k)
            v = np.where(outside[..., None], F(0), v).astype(F)
            n += 1
            if n == 1:
                mean = v
            else:
                with np.errstate(invalid="ignore", over="ignore"):
                    mean = (mean + (v - mean) * (F(1) / F(n))).astype(F)
    return mean


# ---------------------------------------------------------------- 2. the geometry in float64, on its own
def f64_direction(x, y, size, projection, aperture=180.0, basis=None):
    """The world direction of the output POSITION (x, y) (pixel centres at i + 0.5), float64 arrays; None where the fisheye has none."""
    w, h = size
    B = np.eye(3) if basis is None else np.asarray(basis, np.float64).reshape(3, 3)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if projection == "equirect":
        lon, lat = (x / w - 0.5) * 2.0 * np.pi, (y / h - 0.5) * np.pi
        comp = np.stack([np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)], -1)
        inside = np.ones(x.shape, bool)
    else:
        px, py = 2.0 * x / w - 1.0, 2.0 * y / h - 1.0
        rho = np.hypot(px, py)
        theta = rho * np.radians(aperture) / 2.0
        safe = np.where(rho > 0, rho, 1.0)
        comp = np.stack([np.sin(theta) * px / safe, np.sin(theta) * py / safe, np.cos(theta)], -1)
        inside = rho <= 1.0
    return comp @ B, inside


def f64_face_camera(face, N, apron, basis=None):
    """The header's table: (look, up, fov) of face 0 ... 5, float64."""
    B = np.eye(3) if basis is None else np.asarray(basis, np.float64).reshape(3, 3)
    table = {0: (B[0], B[1]), 1: (-B[0], B[1]), 2: (B[1], -B[2]), 3: (-B[1], B[2]), 4: (B[2], B[1]), 5: (-B[2], B[1])}
    look, up = table[face]
    return look, up, N / (N - 2.0 * apron)


def f64_cast_dir(look, up, fov, N, X, Y):
    """The renderer's cast (get_cast_dir with aspect 1, aspect_scale 1) through pixel POSITION (X + 0.5, Y + 0.5) of an N x N camera looking along
    `look`: X, Y are pixel coordinates with integers at the centres, so the jitter is 0.5 plus their fraction.  Without the cast's 1e-5 offset."""
    d = look / np.linalg.norm(look)
    du = np.cross(d, up)
    du = du / np.linalg.norm(du)
    dv = np.cross(du, d)
    dv = dv / np.linalg.norm(dv)
    fu = 2.0 * fov * (np.asarray(X, np.float64) + 0.5) / N - fov
    fv = 2.0 * fov * (np.asarray(Y, np.float64) + 0.5) / N - fov
    v = d + fu[..., None] * du + fv[..., None] * dv
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def f64_linear_faces(N, apron, basis=None):
    """Six faces whose CONTENT has a closed form on the sphere: pixel (u, v) of face k holds the float64 cast direction of its centre divided by the
    direction's component along the face's look, d / (d . look) = look + fu du + fv dv in world coordinates — linear in (u, v) on every face, so a
    correct bilinear tap reproduces it exactly but for float32 rounding.  (6, N, N, 3), rounded to float32 once."""
    idx = np.arange(N, dtype=np.float64)
    X, Y = np.meshgrid(idx, idx, indexing="ij")
    out = np.empty((6, N, N, 3), np.float64)
    for face in range(6):
        look, up, fov = f64_face_camera(face, N, apron, basis)
        d = f64_cast_dir(look, up, fov, N, X, Y)
        out[face] = d / (d @ look)[..., None]
    return out.astype(F)


def f64_linear_image(size, projection, aperture=180.0, basis=None, S=1):
    """What a panorama of f64_linear_faces holds, in float64 and free of any face, tap or table: at an output direction D the value is
    D / max |component of D in the panorama's frame|, in world coordinates — the same on both sides of a cube edge — and 0 beyond the fisheye's
    circle; the mean over the S x S sub-positions of a pixel.  Returns (image (width, height, 3), inside, outside): the pixels all of whose
    sub-positions lie inside the image, and those all of whose lie beyond the circle."""
    w, h = size
    B = np.eye(3) if basis is None else np.asarray(basis, np.float64).reshape(3, 3)
    total = np.zeros((w, h, 3))
    every, none = np.ones((w, h), bool), np.ones((w, h), bool)
    for b in range(S):
        for a in range(S):
            x, y = np.meshgrid(np.arange(w) + (a + 0.5) / S, np.arange(h) + (b + 0.5) / S, indexing="ij")
            d, inside = f64_direction(x, y, size, projection, aperture, basis)
            v = d / np.abs(d @ B.T).max(-1, keepdims=True)
            total += np.where(inside[..., None], v, 0.0)
            every &= inside
            none &= ~inside
    return total / float(S * S), every, none


def f64_major_axis(direction, basis=None):
    """(face, gap): the face of the float64 direction and the difference of its two largest component magnitudes in the panorama's frame."""
    B = np.eye(3) if basis is None else np.asarray(basis, np.float64).reshape(3, 3)
    comp = direction @ B.T
    mag = np.abs(comp)
    axis = mag.argmax(-1)
    srt = np.sort(mag, -1)
    face = 2 * axis + (np.take_along_axis(comp, axis[..., None], -1)[..., 0] < 0)
    return face, srt[..., 2] - srt[..., 1]
