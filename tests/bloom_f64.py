"""A float64 statement of the bloom (include/digital_earth_bloom.h), written from the prose and in another structure than the kernels
and their float32 restatement: no pass over an image, but one dense operator per level and axis, one row per output sample, and the glow as the
linear map G = P b that they compose to.  It shares no code with tests/bloom_ref.py, tests/local_exposure_ref.py or csrc/.

    D_l = Dx_l ... Dx_1  b  (Dy_l ... Dy_1)^T                                  l levels down, separable
    G   = sum_{l=1..L} c_l (Ux_1 ... Ux_l Dx_l ... Dx_1) b (Uy_1 ... Uy_l Dy_l ... Dy_1)^T
    c_l = (1 - spread) spread^(l-1) for l < L,  c_L = spread^(L-1)             the `spread` recursion, unrolled; the c_l sum to 1

so P = sum_l c_l kron(Ax_l, Ay_l) with Ax_l = Ux_1 ... Ux_l Dx_l ... Dx_1 (W x W) and Ay_l likewise (H x H).  `factors` returns the (c_l, Ax_l, Ay_l);
row sums, column sums, signs and the diagonal of P are read off them without forming P (24 960 x 24 960 at 208x120); `dense` forms it where it fits.

The settings and the luminance weights enter as the float32 numbers the interface and the prose hold (`0.2126f`, `1e-5f`, a `float` field); from there on
everything is float64.  Arrays are (W, H, 3) in fetch_hdr's layout: axis 0 is x, axis 1 is y."""
import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
KR, KG, KB, EPS = (float(np.float32(v)) for v in (0.2126, 0.7152, 0.0722, 1e-5))


def _s(v):
    """A setting as the `float` field holds it."""
    return float(np.float32(v))


def plan(W, H, levels):
    """[(W_0, H_0) ... (W_L, H_L)].  §12: every level is ((w + 1) >> 1, (h + 1) >> 1) of the one before; L = levels, reduced so that halving stops
    before a level whose smaller side would be below 2, never less than 1."""
    sizes = [(int(W), int(H))]
    for _ in range(int(levels)):
        w, h = sizes[-1]
        sizes.append(((w + 1) >> 1, (h + 1) >> 1))
    L = max(1, sum(1 for w, h in sizes[1:] if min(w, h) >= 2))      # the sizes never grow, so the levels with both sides >= 2 come first
    return sizes[:L + 1]


def down_matrix(n):
    """((n + 1) >> 1) x n: output x reads columns 2x-1 .. 2x+2, clamped to the level, with 1/8, 3/8, 3/8, 1/8."""
    M = np.zeros(((n + 1) >> 1, n))
    for x in range(M.shape[0]):
        for k, wgt in zip(range(2 * x - 1, 2 * x + 3), (0.125, 0.375, 0.375, 0.125)):
            M[x, min(max(k, 0), n - 1)] += wgt
    return M


def up_matrix(n_fine, n_coarse):
    """n_fine x n_coarse: 3/4 of near = x >> 1 and 1/4 of far = near - 1 (even x) or near + 1 (odd x), clamped to the coarse level."""
    M = np.zeros((n_fine, n_coarse))
    for x in range(n_fine):
        near = x >> 1
        far = near - 1 if x % 2 == 0 else near + 1
        M[x, near] += 0.75
        M[x, min(max(far, 0), n_coarse - 1)] += 0.25
    return M


def axis_chains(ns):
    """For one axis with level sizes ns[0..L]: ([down to level l from level 0], [up from level l to level 0]) for l = 0..L."""
    downs, ups = [np.eye(ns[0])], [np.eye(ns[0])]
    for l in range(1, len(ns)):
        downs.append(down_matrix(ns[l - 1]) @ downs[-1])
        ups.append(ups[-1] @ up_matrix(ns[l - 1], ns[l]))
    return downs, ups


def level_weights(L, spread):
    """c_1 .. c_L: U_L = D_L, U_l = (1 - spread) D_l + spread up(U_{l+1}) for l = L-1 .. 1, G = up(U_1); level 0 is not blended in."""
    s = _s(spread)
    return [(1.0 - s) * s ** (l - 1) for l in range(1, L)] + [s ** (L - 1)]


def factors(W, H, levels, spread):
    """[(c_l, Ax_l, Ay_l)] for l = 1..L with P = sum_l c_l kron(Ax_l, Ay_l)."""
    sizes = plan(W, H, levels)
    L = len(sizes) - 1
    dx, ux = axis_chains([s[0] for s in sizes])
    dy, uy = axis_chains([s[1] for s in sizes])
    return [(c, ux[l] @ dx[l], uy[l] @ dy[l]) for l, c in zip(range(1, L + 1), level_weights(L, spread))]


def dense(fs):
    """P itself, (W H) x (W H), rows and columns indexed x * H + y.  For small sizes only."""
    return sum(c * np.kron(ax, ay) for c, ax, ay in fs)


def row_sums(fs):
    return sum(c * np.outer(ax.sum(axis=1), ay.sum(axis=1)) for c, ax, ay in fs)


def column_sums(fs):
    """(W, H): the total weight every input pixel has over all outputs; 1 everywhere would be conservation of energy."""
    return sum(c * np.outer(ax.sum(axis=0), ay.sum(axis=0)) for c, ax, ay in fs)


def diagonal(fs):
    """(W, H): the weight of a pixel's own value in its own glow."""
    return sum(c * np.outer(np.diag(ax), np.diag(ay)) for c, ax, ay in fs)


def apply(fs, b):
    """G = P b for b of shape (W, H) or (W, H, C)."""
    b = np.asarray(b, dtype=np.float64)
    return sum(c * np.moveaxis(np.tensordot(ay, np.tensordot(ax, b, axes=(1, 0)), axes=(1, 1)), 0, 1) for c, ax, ay in fs)


def _interval_max(a, M):
    """out[i] = max of a[x] over the x with M[i, x] > 0, along axis 0; every row's support is one interval (asserted)."""
    pos = M > 0
    lo, n = pos.argmax(axis=1), pos.sum(axis=1)
    assert (n > 0).all() and all(pos[i, lo[i]:lo[i] + n[i]].all() for i in range(len(lo)))
    padded = np.concatenate([a, np.zeros((1,) + a.shape[1:])])                                 # so that an interval may end at the last sample
    return np.maximum.reduceat(padded, np.stack([lo, lo + n], axis=1).reshape(-1), axis=0)[::2]


def support_max(fs, a):
    """(W, H, C): the largest a[x, y] among the inputs that output (i, j) has a positive weight on.  a >= 0, shape (W, H, C)."""
    a = np.asarray(a, dtype=np.float64)
    out = np.zeros(a.shape)
    for c, ax, ay in fs:
        if c > 0:
            out = np.maximum(out, np.swapaxes(_interval_max(np.swapaxes(_interval_max(a, ax), 0, 1), ay), 0, 1))
    return out


def mean_of(sums, samples):
    """m = sums / count in float64; samples: a scalar, or (W, H) per-pixel counts."""
    n = np.asarray(samples, dtype=np.float64)
    if n.ndim == 2:
        n = n[..., None]
    with np.errstate(all="ignore"):
        return np.asarray(sums, dtype=np.float64) / n


def luminance(m):
    with np.errstate(all="ignore"):
        return (KR * m[..., 0] + KG * m[..., 1]) + KB * m[..., 2]


def bright(m, threshold=0.0, knee=0.5, clamp=0.0):
    """(b, valid, Y).  A pixel is light iff Y > 0 and Y <= FLT_MAX; the others give b = 0."""
    t, k, cl = _s(threshold), _s(knee), _s(clamp)
    Y = luminance(m)
    with np.errstate(all="ignore"):
        valid = (Y > 0) & (Y <= FLT_MAX)
        q = np.minimum(np.maximum((Y - t) + t * k, 0.0), 2.0 * (t * k))
        soft = (q * q) / (4.0 * (t * k) + EPS)
        Yb = np.maximum(soft, Y - t)
        if cl > 0:
            Yb = np.minimum(Yb, cl)
        b = m * (Yb / Y)[..., None]
    return np.where(valid[..., None], b, 0.0), valid, Y


def bloom(sums, samples, intensity=0.05, threshold=0.0, knee=0.5, clamp=0.0, spread=0.7, levels=6, fs=None):
    """(out, G, b, m, valid, Y) in float64; fs: the factors for (W, H, levels, spread) where the caller holds them already."""
    m = mean_of(sums, samples)
    b, valid, Y = bright(m, threshold, knee, clamp)
    if fs is None:
        fs = factors(m.shape[0], m.shape[1], levels, spread)
    G = apply(fs, b)
    with np.errstate(all="ignore"):
        out = m + _s(intensity) * (G - b)
    return out, G, b, m, valid, Y
