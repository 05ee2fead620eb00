"""A numpy float32 restatement of the bloom of the display path (include/digital_earth_bloom.h): the source pixel, its bright part, the
down pyramid, the blended up pyramid and the composite.  It shares no code with csrc/.  Every step is f32 `+ - * /`, min, max and compares in the
order the design states, so the device must give the same bits.  Arrays are (W, H, 3) in fetch_hdr's layout: axis 0 is x ("horizontal"), axis 1 is y."""
import numpy as np

DEFAULTS = dict(intensity=0.05, threshold=0.0, knee=0.5, clamp=0.0, spread=0.7, levels=6)
FLT_MAX = np.finfo(np.float32).max


def _f(x):
    return np.float32(x)


def levels_used(W, H, levels):
    """`levels`, reduced so that halving stops before a level whose smaller side would be below 2; never less than 1."""
    L, w, h = 0, int(W), int(H)
    while L < int(levels):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        if min(w, h) < 2 and L >= 1:
            break
        L += 1
    return L


def level_sizes(W, H, L):
    """[(W_0, H_0), ... (W_L, H_L)]: every level is ((w + 1) >> 1, (h + 1) >> 1) of the one before."""
    out = [(int(W), int(H))]
    for _ in range(L):
        w, h = out[-1]
        out.append(((w + 1) >> 1, (h + 1) >> 1))
    return out


def mean_of(sums, samples):
    """Step 1: the display's own division, f32 sum / f32 count.  samples: a scalar, or (W, H) per-pixel counts (an adaptive frame's tile counts, expanded)."""
    s = np.asarray(sums, dtype=np.float32)
    n = np.asarray(samples).astype(np.float32)
    if n.ndim == 2:
        n = n[..., None]
    with np.errstate(all="ignore"):
        return (s / n).astype(np.float32)


def bright(m, threshold=0.0, knee=0.5, clamp=0.0):
    """Step 2: the part of the mean above the threshold (soft knee, optional clamp), chroma kept.  Pixels whose luminance is not in (0, FLT_MAX] give 0."""
    m = np.asarray(m, dtype=np.float32)
    t, k, cl = _f(threshold), _f(knee), _f(clamp)
    with np.errstate(all="ignore"):
        Y = (_f(0.2126) * m[..., 0] + _f(0.7152) * m[..., 1]) + _f(0.0722) * m[..., 2]
        ok = (Y > 0) & (Y <= FLT_MAX)
        tk = t * k
        q = np.minimum(np.maximum((Y - t) + tk, _f(0)), _f(2) * tk)
        soft = (q * q) / (_f(4) * tk + _f(1e-5))
        Yb = np.maximum(soft, Y - t)
        if cl > 0:
            Yb = np.minimum(Yb, cl)
        w = Yb / Y
        b = m * w[..., None]
    return np.where(ok[..., None], b, _f(0)).astype(np.float32)


def _take(a, idx, axis):
    return np.take(a, idx, axis=axis)


def _down_axis(a, axis):
    n = a.shape[axis]
    x = np.arange((n + 1) >> 1)
    p0, p1, p2, p3 = (_take(a, np.clip(2 * x + k, 0, n - 1), axis) for k in (-1, 0, 1, 2))
    return (_f(0.125) * p0 + _f(0.375) * p1) + (_f(0.375) * p2 + _f(0.125) * p3)


def down(a):
    """Step 3: one level down, horizontal first, indices clamped to the level."""
    return _down_axis(_down_axis(np.asarray(a, dtype=np.float32), 0), 1)


def _up_axis(a, n_fine, axis):
    x = np.arange(n_fine)
    near = x >> 1
    far = np.clip(np.where(x & 1, near + 1, near - 1), 0, a.shape[axis] - 1)
    return _f(0.75) * _take(a, near, axis) + _f(0.25) * _take(a, far, axis)


def up(a, size):
    """Step 5's `up`: to `size` = (W_fine, H_fine), horizontal first."""
    return _up_axis(_up_axis(np.asarray(a, dtype=np.float32), size[0], 0), size[1], 1)


def glow(b, spread=0.7, levels=6):
    """Steps 3-5: G at full resolution from the bright part b (W, H, 3)."""
    W, H = b.shape[:2]
    L = levels_used(W, H, levels)
    sizes = level_sizes(W, H, L)
    D = [np.asarray(b, dtype=np.float32)]
    for _ in range(L):
        D.append(down(D[-1]))
    s = _f(spread)
    U = D[L]
    for l in range(L - 1, 0, -1):
        U = (_f(1) - s) * D[l] + s * up(U, sizes[l])
    return up(U, sizes[0])


def bloom(sums, samples, intensity=0.05, threshold=0.0, knee=0.5, clamp=0.0, spread=0.7, levels=6):
    """Steps 1-6.  sums: (W, H, 3) float32; samples: spp, or (W, H) per-pixel counts.  Returns (out, G, b)."""
    m = mean_of(sums, samples)
    b = bright(m, threshold, knee, clamp)
    G = glow(b, spread, levels)
    with np.errstate(all="ignore"):
        out = m + _f(intensity) * (G - b)
    return out.astype(np.float32), G, b
