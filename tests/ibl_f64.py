"""An independent float64 statement of the IBL bake's mathematics (include/digital_earth_ibl.h).  It shares no code with
tests/ibl_ref.py: directions, the lookup, the GGX estimator and the SH quadrature are written again, in float64, from the header's text.

    cube_dirs(e)                    unit directions of the texel centres, (6, e, e, 3)
    solid_angles(e)                 the corner formula, (e, e) float64
    sh_quadrature(level)            sum over texels of value * Y_b * dw, times the cosine lobe: (3, 9) float64
    real_sh(d)                      Y_0 ... Y_8 at unit directions
    specular(chain, L, K, l, bias)  the filtered importance-sampled GGX estimator of level l, (6, e, e, 3) float64
"""
import numpy as np

PI = np.pi
LOBE = np.array([PI] + [2.0 * PI / 3.0] * 3 + [PI / 4.0] * 5)


def _face_vec(face, a, b):
    one = np.ones_like(a)
    table = {0: (one, -b, -a), 1: (-one, -b, a), 2: (a, one, b), 3: (a, -one, -b), 4: (a, -b, one), 5: (-a, -b, -one)}
    return np.stack(table[face], -1)


def cube_dirs(e):
    c = (2.0 * np.arange(e) + 1.0) / e - 1.0
    a, b = np.meshgrid(c, c, indexing="xy")      # a along the columns, b along the rows
    d = np.stack([_face_vec(f, a, b) for f in range(6)])
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def solid_angles(e):
    g = 2.0 * np.arange(e + 1) / e - 1.0
    x, y = np.meshgrid(g, g, indexing="xy")
    A = np.arctan2(x * y, np.sqrt(x * x + y * y + 1.0))
    return A[1:, 1:] - A[1:, :-1] - A[:-1, 1:] + A[:-1, :-1]


def real_sh(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    k1, k2 = np.sqrt(3.0 / (4.0 * PI)), np.sqrt(15.0 / (4.0 * PI))
    return np.stack([np.full_like(x, np.sqrt(1.0 / (4.0 * PI))), k1 * y, k1 * z, k1 * x, k2 * x * y, k2 * y * z,
                     np.sqrt(5.0 / (16.0 * PI)) * (3.0 * z * z - 1.0), k2 * x * z, 0.5 * k2 * (x * x - y * y)], -1)


def sh_quadrature(level):
    level = np.asarray(level, np.float64)
    e = level.shape[1]
    w = real_sh(cube_dirs(e)) * solid_angles(e)[None, :, :, None]
    return np.einsum("fjic,fjib->cb", level, w) * LOBE[None, :]


def _fetch(level, d, face=None):
    e = level.shape[1]
    mag = np.abs(d)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    if face is None:
        r = (mag[..., 0] >= mag[..., 1]) & (mag[..., 0] >= mag[..., 2])
        u = ~r & (mag[..., 1] >= mag[..., 2])
        face = np.where(r, np.where(x < 0, 1, 0), np.where(u, np.where(y < 0, 3, 2), np.where(z < 0, 5, 4)))
    ma = np.take_along_axis(mag, (face // 2)[..., None], -1)[..., 0]
    sc = np.select([face == 0, face == 1, face == 5], [-z, z, -x], x) / ma
    tc = np.select([face == 2, face == 3], [z, -z], -y) / ma
    X = np.clip((sc + 1.0) * e / 2.0 - 0.5, 0.0, e - 1.0)
    Yc = np.clip((tc + 1.0) * e / 2.0 - 0.5, 0.0, e - 1.0)
    i0, j0 = np.floor(X).astype(int), np.floor(Yc).astype(int)
    i1, j1 = np.minimum(i0 + 1, e - 1), np.minimum(j0 + 1, e - 1)
    fx, fy = (X - i0)[..., None], (Yc - j0)[..., None]
    top = level[face, j0, i0] * (1.0 - fx) + level[face, j0, i1] * fx
    bottom = level[face, j1, i0] * (1.0 - fx) + level[face, j1, i1] * fx
    return top * (1.0 - fy) + bottom * fy


def _van_der_corput(k):
    v, f = 0.0, 0.5
    while k:
        v += f * (k & 1)
        k >>= 1
        f *= 0.5
    return v


def specular(chain, L, K, l, lod_bias=0.0, faces=None):
    """faces: optionally, per KEPT sample in order, the face (6, e, e) its lookup reads — decided elsewhere where a direction lies on a cube edge."""
    chain = [np.asarray(c, np.float64) for c in chain]
    E = chain[0].shape[1]
    M = len(chain)
    e = E >> l
    alpha = (l / (L - 1.0)) ** 2
    N = cube_dirs(e)
    steep = np.abs(N[..., 1]) >= np.float32(0.999)
    up = np.where(steep[..., None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    T = np.cross(up, N)
    T /= np.linalg.norm(T, axis=-1, keepdims=True)
    B = np.cross(N, T)
    total, weight, kept = np.zeros(N.shape), 0.0, 0
    for k in range(K):
        u1, u2 = (k + 0.5) / K, _van_der_corput(k)
        cos2 = (1.0 - u1) / (1.0 + (alpha ** 2 - 1.0) * u1)
        sin_t, phi = np.sqrt(1.0 - cos2), 2.0 * PI * u2
        h = np.array([sin_t * np.cos(phi), sin_t * np.sin(phi), np.sqrt(cos2)])
        H = T * h[0] + B * h[1] + N * h[2]
        Ld = 2.0 * h[2] * H - N
        n_dot_l = 2.0 * cos2 - 1.0
        if n_dot_l <= 0.0:
            continue
        D = alpha ** 2 / (PI * (cos2 * (alpha ** 2 - 1.0) + 1.0) ** 2)
        lod = max(0.0, 0.5 * np.log2((1.0 / (K * D / 4.0)) / (4.0 * PI / (6.0 * E * E)))) + float(np.float32(lod_bias))
        lod = min(max(lod, 0.0), M - 1.0)
        lo = min(int(np.floor(lod)), M - 1)
        hi = min(lo + 1, M - 1)
        f = lod - lo
        face = None if faces is None else faces[kept]
        kept += 1
        v = _fetch(chain[lo], Ld, face) * (1.0 - f) + _fetch(chain[hi], Ld, face) * f
        total += v * n_dot_l
        weight += n_dot_l
    return total / weight
