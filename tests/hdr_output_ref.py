"""A numpy float32 restatement of the HDR display output (include/digital_earth_hdr_output.h): the constants of a setting, openDR_transform
in its general form (lib/OpenDRT.py:221-485: peak luminance, display gamut, inverse EOTF), the display around it, and the 10 / 16-bit pack.  Written from
the header, the design and the reference's formulas; it shares no code with csrc/.  Every step is f32 `+ - * /`, min, max and compares in the reference's
order, plus a power, a logarithm and a square root that are PARAMETERS: on the CPU they default to numpy's float32 routines called value by value, as the
executed reference calls them (tools/ref_fixtures/make_hdr.py); the GPU tests pass the device's own de_pow, de_log and de_sqrt (Renderer.debug_math), and then
the device must give the same bits.  The hash of the dither is tests/pixels_ref.py's.  Images are (W, H, 3) in fetch_hdr's layout."""
import math

import numpy as np

import pixels_ref

GAMUTS = ("rec709", "p3d65", "rec2020")
TRANSFERS = ("linear", "pq", "hlg")
FORMATS = ("rgb10a2", "rgb16")
MODES = pixels_ref.MODES
DEFAULTS = dict(on=True, peak_nits=1000.0, gamut="rec2020", transfer="pq", pixel_format="rgb10a2", mode="truncate", seed=0, animate=False)
MAXCODE = {"rgb10a2": 1023, "rgb16": 65535}
CICP = {"rec709": 1, "p3d65": 12, "rec2020": 9}, {"linear": 8, "pq": 16, "hlg": 18}      # colour primaries, transfer characteristics (ITU-T H.273)
F = np.float32
U = np.uint32

REC709_TO_XYZ = (0.412390917540, 0.357584357262, 0.180480793118, 0.212639078498, 0.715168714523, 0.072192311287, 0.019330825657, 0.119194783270, 0.950532138348)
XYZ_TO = {
    "rec709": (3.2409699419, -1.53738317757, -0.498610760293, -0.969243636281, 1.87596750151, 0.041555057407, 0.055630079697, -0.203976958889, 1.05697151424),
    "p3d65": (2.49349691194, -0.931383617919, -0.402710784451, -0.829488969562, 1.76266406032, 0.023624685842, 0.035845830244, -0.076172389268, 0.956884524008),
    "rec2020": (1.71665118797, -0.355670783776, -0.253366281374, -0.666684351832, 1.61648123664, 0.015768545814, 0.017639857445, -0.042770613258, 0.942103121235),
}


# ---------------------------------------------------------------------------------------------- the elementary functions' defaults
def _each(fn, *xs):
    xs = np.broadcast_arrays(*[np.asarray(x, dtype=F) for x in xs])
    out = np.empty(xs[0].shape, F)
    with np.errstate(all="ignore"):
        for k in np.ndindex(out.shape):
            out[k] = fn(*[x[k] for x in xs])
    return out


def pow_np(x, y):
    """numpy's float32 power, one value at a time (the scalar routine: the array loops may take another one)."""
    return _each(np.power, x, y)


def log_np(x):
    return _each(np.log, x)


def sqrt_np(x):
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(x, dtype=F))      # correctly rounded wherever it runs


# ---------------------------------------------------------------------------------------------- the constants of a setting
def constants(peak_nits=1000.0, gamut="rec2020", transfer="pq"):
    """What de_set_hdr_output computes on the host in double and rounds to f32 (lib/OpenDRT.py:270-271, 306-319, 404; :72-74; :140-146)."""
    Lp, gb, c, fl, dch = float(F(peak_nits)), 0.12, 1.0, 0.005, 0.35
    ds = 0.01 if transfer == "pq" else (0.1 if transfer == "hlg" else 100.0 / Lp)
    clamp_max = ds * Lp / 100.0
    px = 128.0 * math.log10(Lp) / math.log10(100.0) - 64.0
    py, gx = Lp / 100.0, 0.18
    gy = 11.696 / 100.0 * (1.0 + gb * math.log10(py) / math.log10(2.0))
    s0 = (gy + math.sqrt(gy * (4.0 * fl + gy))) / 2.0
    m0 = (py + math.sqrt(py * (4.0 * fl + py))) / 2.0
    ip = 1.0 / c
    s = (px * gx * (m0 ** ip - s0 ** ip)) / (px * s0 ** ip - gx * m0 ** ip)
    m = m0 ** ip * (s + px) / px
    h_a = 0.17883277
    h_b = 1.0 - 4.0 * 0.17883277
    h_c = 0.5 - h_a * math.log10(4.0 * h_a)
    h_g = 1.2 * math.pow(1.111, math.log2(1000.0 / 1000.0)) * math.pow(0.98, math.log2(max(1e-6, 5.0) / 5.0))
    return dict(m=F(m), s=F(s), fl=F(fl), ds=F(ds), clamp_max=F(clamp_max), dch_s=F(dch / s), xyz_to_display=np.array(XYZ_TO[gamut], F),
                h_a=F(h_a), h_b=F(h_b), h_c=F(h_c), h_e=F((1.0 - h_g) / h_g))


def constants_vector(k):
    """The 19 floats of de_debug_hdr_consts."""
    return np.concatenate([[k["m"], k["s"], k["fl"], k["ds"], k["clamp_max"], k["dch_s"]], k["xyz_to_display"], [k["h_a"], k["h_b"], k["h_c"], k["h_e"]]]).astype(F)


# ---------------------------------------------------------------------------------------------- the transform
def _max(a, b):
    """(b > a) ? b : a"""
    return np.where(b > a, b, a).astype(F)


def _min(a, b):
    """(b < a) ? b : a"""
    return np.where(b < a, b, a).astype(F)


def _sdiv(a, b):
    """sdivf (lib/OpenDRT.py:92-97): 0 where |b| < 1e-4."""
    small = np.abs(b) < F(1e-4)
    return np.where(small, F(0), a / np.where(small, F(1), b)).astype(F)


def _vdot(m, v):
    """v @ m (lib/OpenDRT.py:86-88), a left fold per output."""
    m = [F(x) for x in m]
    return [(v[0] * m[j] + v[1] * m[3 + j]) + v[2] * m[6 + j] for j in range(3)]


def _narrow(v):
    two, zero = F(2), F(0)
    return [_min(two, _max(zero, v[0] - (v[1] + v[2]))), _min(two, _max(zero, v[1] - (v[0] + v[2]))), _min(two, _max(zero, v[2] - (v[0] + v[1])))]


def pq_inverse_eotf(x, pow=pow_np):
    """eotf_pq(rgb, 1), lib/OpenDRT.py:166-184, one channel."""
    m1, m2, c1, c2, c3 = F(2610.0 / 16384.0), F(2523.0 / 32.0), F(107.0 / 128.0), F(2413.0 / 128.0), F(2392.0 / 128.0)
    a = np.asarray(pow(x, np.full(np.shape(x), m1, F)), F)
    q = ((c1 + c2 * a) / (F(1) + c3 * a)).astype(F)
    return np.asarray(pow(q, np.full(np.shape(x), m2, F)), F)


def _log10(x, log):
    return ((np.asarray(log(x), F) / F(math.log(2.0))) / F(math.log(10.0) / math.log(2.0))).astype(F)


def hlg_inverse_eotf(rgb, k, pow=pow_np, log=log_np, sqrt=sqrt_np):
    """eotf_hlg(rgb, 1), lib/OpenDRT.py:133-155; rgb a list of three arrays."""
    Yd = (F(0.2627) * rgb[0] + F(0.6780) * rgb[1]) + F(0.0593) * rgb[2]
    g = np.asarray(pow(Yd, np.full(np.shape(Yd), k["h_e"], F)), F)
    out = []
    for x in rgb:
        x = (x * g).astype(F)
        low = x <= F(1.0 / 12.0)      # a NaN takes the logarithm's branch, as on the device
        y = np.empty(x.shape, F)
        if low.any():
            y[low] = np.asarray(sqrt(F(3) * x[low]), F)
        if (~low).any():
            y[~low] = k["h_a"] * _log10(F(12) * x[~low] - k["h_b"], log) + k["h_c"]
        out.append(y)
    return out


def transform(rgb, peak_nits=1000.0, gamut="rec2020", transfer="pq", pow=pow_np, log=log_np, sqrt=sqrt_np, consts=None):
    """openDR_transform on (..., 3) scene-linear Rec.709 colours, already exposed.  Returns the signal, float32 of the same shape."""
    k = constants(peak_nits, gamut, transfer) if consts is None else consts
    x = np.asarray(rgb, dtype=F)
    shape = x.shape
    x = x.reshape(-1, 3)
    with np.errstate(all="ignore"):
        v = _vdot(REC709_TO_XYZ, [x[:, 0], x[:, 1], x[:, 2]])
        v = _vdot(k["xyz_to_display"], v)
        mx = _max(v[0], _max(v[1], v[2]))
        mn = _min(v[0], _min(v[1], v[2]))
        h_rgb = _narrow([_sdiv(c - mn, mx) for c in v])
        w0 = np.array([0.25, 1.0, 0.35], F)
        w0 = w0 / np.asarray(sqrt(np.array([(w0[0] * w0[0] + w0[1] * w0[1]) + w0[2] * w0[2]], F)), F)[0]
        w = [w0[i] * _max(v[i], F(1e-5)) for i in range(3)]
        lum = np.asarray(sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]), F)
        rats = [_sdiv(c, lum) for c in v]
        ts = k["m"] * lum / (lum + k["s"])
        ts = np.where(ts <= 0, ts, ts * ts) / (ts + k["fl"])
        ts = (ts * k["ds"]).astype(F)
        ccf = _sdiv(F(1), lum * k["dch_s"] + F(1))
        toe_ccf = _sdiv(lum, lum + F(0)) * ccf
        hs_w = [(F(1) - ccf) * c for c in h_rgb]
        hs_r, hs_g, hs_b = F(0.3), F(-0.1), F(-0.2)
        rats = [rats[0] + hs_w[2] * hs_b - hs_w[1] * hs_g, rats[1] + hs_w[0] * hs_r - hs_w[2] * hs_b, rats[2] + hs_w[1] * hs_g - hs_w[0] * hs_r]
        rats = [_max(F(1) - toe_ccf + c * toe_ccf, F(0)) for c in rats]
        rmx = _max(rats[0], _max(rats[1], rats[2]))
        rmn = _min(rats[0], _min(rats[1], rats[2]))
        chf_in = (_sdiv(rmx - rmn, rmx) * ts).astype(F)
        chf = chf_in.copy()
        pos = ~(chf_in <= 0)
        if pos.any():
            chf[pos] = np.asarray(sqrt(chf_in[pos]), F)
        rats_n = [_sdiv(c, rmx) for c in rats]
        rats = [n * chf + c * (F(1) - chf) for n, c in zip(rats_n, rats)]
        out = [_min(c * ts, k["clamp_max"]) for c in rats]
        if transfer == "pq":
            out = [pq_inverse_eotf(c, pow) for c in out]
        elif transfer == "hlg":
            out = hlg_inverse_eotf(out, k, pow, log, sqrt)
        elif transfer != "linear":
            raise ValueError(transfer)
    return np.stack(out, axis=-1).astype(F).reshape(shape)


def display_linear(sums, samples, exposure_scale, vignette=(0.9, 0.0, 0.5, 0.5), sqrt=sqrt_np):
    """What the stage reads: the frame's mean, vignetted and exposed (renderer.py:349-355), display-linear.  Arguments as display()."""
    sums = np.asarray(sums, F)
    W, H = sums.shape[:2]
    n = np.asarray(samples).astype(F)
    if n.ndim == 2:
        n = n[..., None]
    strength, radius, cx, cy = (F(x) for x in vignette)
    with np.errstate(all="ignore"):
        u = (np.arange(W).astype(F) / F(W))[:, None]
        v = (np.arange(H).astype(F) / F(H))[None, :]
        du, dv = u - cx, v - cy
        dist = np.asarray(sqrt((du * du + dv * dv).astype(F)), F)
        darken = F(1) - strength * _max(dist - radius, F(0))
        linear = ((sums / n) * darken[..., None]) * F(exposure_scale)
    return linear.astype(F)


def display(sums, samples, exposure_scale, vignette=(0.9, 0.0, 0.5, 0.5), sqrt=sqrt_np, **kw):
    """The stage on a frame: sums (W, H, 3) in fetch_hdr's layout, samples a count or (W, H) per-pixel counts, exposure_scale the display's 2^exposure,
    vignette = (strength, radius, centre x, centre y) (renderer.py:349-355).  kw: transform's."""
    return transform(display_linear(sums, samples, exposure_scale, vignette, sqrt), sqrt=sqrt, **kw)


# ---------------------------------------------------------------------------------------------- the pack
def quantise(t, maxcode, mode, seed=0, phase=0, idx=None):
    """pixels_ref.quantise with 255 replaced by maxcode."""
    t = np.asarray(t, dtype=F)
    mc = F(maxcode)
    with np.errstate(invalid="ignore"):
        cl = np.where(t > F(0), np.where(t < F(1), t, F(1)), F(0)).astype(F)
    s = cl * mc
    if mode == "truncate":
        return s.astype(np.int32).astype(np.int64)
    if mode == "round":
        return (s + F(0.5)).astype(np.int32).astype(np.int64)
    if mode != "dither":
        raise ValueError(mode)
    e = mc - s
    m = np.where(s < e, s, e).astype(F)
    a = np.where(m < F(1), m, F(1)).astype(F)
    return ((s + F(0.5)) + a * pixels_ref.tri(seed, phase, idx)).astype(F).astype(np.int32).astype(np.int64)


def pack(image, pixel_format="rgb10a2", mode="truncate", seed=0, phase=0):
    """(W, H, 3) float32 signal -> uint32 (H, W) (R bits 0-9, G 10-19, B 20-29, alpha 3 in 30-31) or uint16 (H, W, 3); row 0 at the top."""
    image = np.asarray(image, dtype=F)
    W, H = image.shape[:2]
    assert image.shape == (W, H, 3)
    mc = MAXCODE[pixel_format]
    q = quantise(image, mc, mode, seed, phase, pixels_ref.indices(W, H) if mode == "dither" else None)
    assert q.min() >= 0 and q.max() <= mc
    q = q.transpose(1, 0, 2)[::-1]      # out[r][x] = image[x][H - 1 - r]
    if pixel_format == "rgb16":
        return np.ascontiguousarray(q.astype(np.uint16))
    return np.ascontiguousarray((q[..., 0] | (q[..., 1] << 10) | (q[..., 2] << 20) | (3 << 30)).astype(np.uint32))


def pq_nits(nits):
    """ST 2084 inverse EOTF of an absolute luminance in float64: the closed form the anchors are held to."""
    m1, m2, c1, c2, c3 = 2610.0 / 16384.0, 2523.0 / 32.0, 107.0 / 128.0, 2413.0 / 128.0, 2392.0 / 128.0
    y = (float(nits) / 10000.0) ** m1
    return ((c1 + c2 * y) / (1.0 + c3 * y)) ** m2
