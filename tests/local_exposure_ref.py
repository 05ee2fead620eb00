"""A numpy float32 restatement of the local exposure of the display path (include/digital_earth_local_exposure.h): luminance and
validity, the weighted pyramid down, the base by joint-bilateral upsampling, the anchor and the gain.  It shares no code with csrc/.  Every step is
f32 `+ - * /`, min, max and compares in the order the design states, plus a logarithm and a power of two that are PARAMETERS: on the CPU they default
to float64 numpy rounded to f32; the GPU tests pass the device's own deterministic de_log and de_pow (Renderer.debug_math), and then the device must
give the same bits.  Arrays are (W, H, 3) in fetch_hdr's layout: axis 0 is x ("horizontal"), axis 1 is y."""
import numpy as np

DEFAULTS = dict(highlights=0.5, shadows=0.25, sigma=1.0, max_ev=2.0, key=0.18, levels=6)
FLT_MAX = np.finfo(np.float32).max
Y_MIN = np.float32(2.0 ** -24)
LOG2E = np.float32(float.fromhex("0x1.715476p+0"))


def _f(x):
    return np.float32(x)


def log_f64(x):
    """Natural logarithm in float64, rounded to f32."""
    with np.errstate(all="ignore"):
        return np.log(np.asarray(x, dtype=np.float64)).astype(np.float32)


def pow2_f64(x):
    """2^x in float64, rounded to f32."""
    return np.exp2(np.asarray(x, dtype=np.float64)).astype(np.float32)


def levels_used(W, H, levels):
    """`levels`, reduced so that halving stops before a level whose smaller side would be below 2; never less than 1 (the bloom's rule)."""
    L, w, h = 0, int(W), int(H)
    while L < int(levels):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        if min(w, h) < 2 and L >= 1:
            break
        L += 1
    return L


def mean_of(sums, samples):
    """The display's own division, f32 sum / f32 count.  samples: a scalar, or (W, H) per-pixel counts (an adaptive frame's tile counts, expanded)."""
    s = np.asarray(sums, dtype=np.float32)
    n = np.asarray(samples).astype(np.float32)
    if n.ndim == 2:
        n = n[..., None]
    with np.errstate(all="ignore"):
        return (s / n).astype(np.float32)


def log_luminance(m, log=log_f64):
    """Step 1: (l, valid).  l is 0 where the pixel is not valid."""
    m = np.asarray(m, dtype=np.float32)
    with np.errstate(all="ignore"):
        Y = (_f(0.2126) * m[..., 0] + _f(0.7152) * m[..., 1]) + _f(0.0722) * m[..., 2]
        valid = (Y >= Y_MIN) & (Y <= FLT_MAX)
    l = np.zeros(Y.shape, np.float32)
    if valid.any():
        l[valid] = (np.asarray(log(Y[valid]), dtype=np.float32) * LOG2E).astype(np.float32)
    return l, valid


def _down_axis(a, axis):
    n = a.shape[axis]
    x = np.arange((n + 1) >> 1)
    p0, p1, p2, p3 = (np.take(a, np.clip(2 * x + k, 0, n - 1), axis=axis) for k in (-1, 0, 1, 2))
    return (_f(0.125) * p0 + _f(0.375) * p1) + (_f(0.375) * p2 + _f(0.125) * p3)


def down(a):
    """Step 2: one level down, horizontal first, indices clamped to the level; a is (w, h, 2) = (l w, w)."""
    return _down_axis(_down_axis(np.asarray(a, dtype=np.float32), 0), 1)


def _guide(D):
    """(guide, counts): D.x / D.y where D.y > 0, else 0."""
    on = D[..., 1] > 0
    g = np.zeros(on.shape, np.float32)
    g[on] = D[..., 0][on] / D[..., 1][on]
    return g, on


def _near_far(n_fine, n_coarse):
    x = np.arange(n_fine)
    near = x >> 1
    far = np.clip(np.where(x & 1, near + 1, near - 1), 0, n_coarse - 1)
    return near, far


def upsample(guide, on, Dc, Bc, sigma):
    """Step 3: the base of a level from the coarser one.  guide, on: (w, h) of the finer level; Dc (wc, hc, 2) and Bc (wc, hc) of the coarser one."""
    gc, onc = _guide(Dc)
    w, h = guide.shape
    xn, xf = _near_far(w, Dc.shape[0])
    yn, yf = _near_far(h, Dc.shape[1])
    inv_sigma = _f(1) / _f(sigma)
    num = np.zeros((w, h), np.float32)
    den = np.zeros((w, h), np.float32)
    with np.errstate(all="ignore"):
        for kx, ky, xi, yi in ((0.75, 0.75, xn, yn), (0.25, 0.75, xf, yn), (0.75, 0.25, xn, yf), (0.25, 0.25, xf, yf)):
            k = _f(kx) * _f(ky)
            tg, tb, ton = gc[np.ix_(xi, yi)], Bc[np.ix_(xi, yi)], onc[np.ix_(xi, yi)]
            a = (guide - tg) * inv_sigma
            r = _f(1) / (_f(1) + a * a)
            wgt = k * r
            num = np.where(ton, num + wgt * tb, num)
            den = np.where(ton, den + wgt, den)
        assert (den[on] > 0).all()      # a pixel with a positive weight lies inside its near tap's footprint
        B = np.zeros((w, h), np.float32)
        B[on] = num[on] / den[on]
    return B


def base(l, valid, sigma=1.0, levels=6):
    """Steps 2 and 3: B_0 (W, H) from l and the validity mask; 0 where the pixel is not valid."""
    W, H = l.shape
    L = levels_used(W, H, levels)
    D = [np.stack([np.where(valid, l, _f(0)), valid.astype(np.float32)], axis=-1).astype(np.float32)]
    for _ in range(L):
        D.append(down(D[-1]))
    B = _guide(D[L])[0]
    for lv in range(L - 1, -1, -1):
        g, on = _guide(D[lv])
        B = upsample(g, on, D[lv + 1], B, sigma)
    return B


def anchor(exposure_scale, key=0.18, log=log_f64):
    """Step 4: the scene luminance that the display maps to the key, in stops."""
    q = np.array([_f(key) / _f(exposure_scale)], np.float32)
    return _f((np.asarray(log(q), dtype=np.float32) * LOG2E)[0])


def gain(B, valid, mid, highlights=0.5, shadows=0.25, max_ev=2.0, pow2=pow2_f64):
    """Step 5: the gain per pixel, 1 where the pixel is not valid or ev == 0."""
    with np.errstate(all="ignore"):
        s = np.where(B > mid, _f(highlights), _f(shadows)).astype(np.float32)
        ev = -(s * (B - mid))
        ev = np.minimum(np.maximum(ev, -_f(max_ev)), _f(max_ev)).astype(np.float32)
    g = np.ones(B.shape, np.float32)
    use = valid & (ev != 0)
    if use.any():
        g[use] = np.asarray(pow2(ev[use]), dtype=np.float32)
    return g


def local_exposure(sums, samples, exposure_scale, highlights=0.5, shadows=0.25, sigma=1.0, max_ev=2.0, key=0.18, levels=6, log=log_f64, pow2=pow2_f64):
    """Steps 1-5.  sums: (W, H, 3) float32; samples: spp, or (W, H) per-pixel counts; exposure_scale: the display's 2^exposure.  Returns (out, gain)."""
    m = mean_of(sums, samples)
    l, valid = log_luminance(m, log)
    B = base(l, valid, sigma, levels)
    mid = anchor(exposure_scale, key, log)
    g = gain(B, valid, mid, highlights, shadows, max_ev, pow2)
    with np.errstate(all="ignore"):
        out = np.where(valid[..., None], m * g[..., None], m).astype(np.float32)
    return out, g
