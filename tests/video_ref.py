"""The video frame output (include/digital_earth_video.h) restated in numpy: uint32 and float32 only on the value path, every operation
in the order the header states, so that the device's bytes can be held to it exactly.

    pack(image, format, matrix, range, siting, mode, seed, phase)  ->  the frame, a flat uint8 array (planes one after the other, rows top-down)
    planes(frame, W, H, format)                                    ->  (Y, Cb, Cr) codes as 2-D integer arrays, whatever the layout

image is the display's output: (W, H, 3) float32, image[u, v] with v = 0 at the bottom; W and H even."""
import numpy as np

import pixels_ref as px

FORMATS = ("nv12", "i420", "p010", "i010")
MATRICES = ("bt709", "bt601", "bt2020")
RANGES = ("limited", "full")
SITINGS = ("left", "center", "topleft")
MODES = px.MODES
DEFAULTS = dict(format="nv12", matrix="bt709", range="limited", siting="left", mode="round", seed=0, animate=False)
KR = {"bt709": 0.2126, "bt601": 0.299, "bt2020": 0.2627}
KB = {"bt709": 0.0722, "bt601": 0.114, "bt2020": 0.0593}
F = np.float32
U = np.uint32


def bits(format):
    return 10 if format in ("p010", "i010") else 8


def consts(format, matrix, range):
    """The kernel's constants: evaluated in double, rounded to f32; kg alone is two f32 operations."""
    Kr, Kb = KR[matrix], KB[matrix]
    k = 4.0 if bits(format) == 10 else 1.0
    M = 1023.0 if bits(format) == 10 else 255.0
    c = dict(kr=F(Kr), kb=F(Kb), sb=F(0.5 / (1.0 - Kb)), sr=F(0.5 / (1.0 - Kr)))
    c["kg"] = F(F(1.0) - F(c["kr"] + c["kb"]))
    if range == "limited":
        c.update(ys=F(219.0 * k), yo=F(16.0 * k), ylo=F(16.0 * k), yhi=F(235.0 * k), cs=F(224.0 * k), co=F(128.0 * k), clo=F(16.0 * k), chi=F(240.0 * k))
    else:
        c.update(ys=F(M), yo=F(0.0), ylo=F(0.0), yhi=F(M), cs=F(M), co=F(128.0 * k), clo=F(0.0), chi=F(M))
    return c


def clamp01(t):
    t = np.asarray(t, dtype=F)
    with np.errstate(invalid="ignore"):
        return np.where(t > F(0), np.where(t < F(1), t, F(1)), F(0)).astype(F)


def ycc(image, c):
    """Per pixel, in the picture's orientation [r][x] (rows top-down): Y, Cb, Cr as f32."""
    rgb = clamp01(image).transpose(1, 0, 2)[::-1]      # [r][x][ch] = image[x][H - 1 - r]
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    Y = (((c["kr"] * R).astype(F) + (c["kb"] * B).astype(F)).astype(F) + (c["kg"] * G).astype(F)).astype(F)
    Cb = ((B - Y).astype(F) * c["sb"]).astype(F)
    Cr = ((R - Y).astype(F) * c["sr"]).astype(F)
    return Y, Cb, Cr


def subsample(c, siting):
    """The siting's filter of one full-resolution difference c[r][x] -> [H / 2][W / 2], taps outside the image repeating the edge pixel."""
    c = np.asarray(c, dtype=F)
    e = np.pad(c, ((1, 0), (1, 0)), mode="edge")       # e[r + 1][x + 1] = c[r][x]; row -1 and column -1 repeat row 0 and column 0
    if siting == "center":
        h = (c[:, 0::2] + c[:, 1::2]).astype(F)        # h[r][i] = c(2i, r) + c(2i + 1, r)
        return ((h[0::2] + h[1::2]).astype(F) * F(0.25)).astype(F)
    h = ((e[:, 0:-1:2] + e[:, 2::2]).astype(F) + (F(2.0) * e[:, 1::2]).astype(F)).astype(F)      # rows -1 ... H - 1: h[r + 1][i] = (c(2i - 1) + c(2i + 1)) + 2 c(2i)
    if siting == "left":
        return ((h[1::2] + h[2::2]).astype(F) * F(0.125)).astype(F)                                # h(2j) + h(2j + 1)
    if siting != "topleft":
        raise ValueError(siting)
    return (((h[0:-1:2] + h[2::2]).astype(F) + (F(2.0) * h[1::2]).astype(F)).astype(F) * F(0.0625)).astype(F)      # (h(2j - 1) + h(2j + 1)) + 2 h(2j)


def clip(v, lo, hi):
    v = np.asarray(v, dtype=F)
    return np.where(v > lo, np.where(v < hi, v, hi), lo).astype(F)


def quantise(s, lo, hi, mode, seed, phase, plane):
    """A plane of clipped values s[row][col] to codes (int64); the dither's idx = 4 (row-major sample index) + plane."""
    s = np.asarray(s, dtype=F)
    if mode == "truncate":
        return s.astype(np.int32).astype(np.int64)
    if mode == "round":
        return (s + F(0.5)).astype(F).astype(np.int32).astype(np.int64)
    if mode != "dither":
        raise ValueError(mode)
    n = np.arange(s.size, dtype=np.int64).reshape(s.shape)
    idx = ((n * 4 + plane) & 0xffffffff).astype(U)
    d, e = (s - lo).astype(F), (hi - s).astype(F)
    m = np.where(d < e, d, e).astype(F)
    a = np.where(m < F(1), m, F(1)).astype(F)
    return ((s + F(0.5)).astype(F) + (a * px.tri(seed, phase, idx)).astype(F)).astype(F).astype(np.int32).astype(np.int64)


def prequant(image, format="nv12", matrix="bt709", range="limited", siting="left"):
    """The three planes' clipped f32 values ahead of the quantiser, and their (lo, hi)."""
    c = consts(format, matrix, range)
    Y, Cb, Cr = ycc(image, c)
    y = clip((Y * c["ys"]).astype(F) + c["yo"], c["ylo"], c["yhi"])
    cb = clip((subsample(Cb, siting) * c["cs"]).astype(F) + c["co"], c["clo"], c["chi"])
    cr = clip((subsample(Cr, siting) * c["cs"]).astype(F) + c["co"], c["clo"], c["chi"])
    return (y, cb, cr), ((c["ylo"], c["yhi"]), (c["clo"], c["chi"]), (c["clo"], c["chi"]))


def codes(image, format="nv12", matrix="bt709", range="limited", siting="left", mode="round", seed=0, phase=0):
    """(Y, Cb, Cr) integer codes: [H][W], [H / 2][W / 2], [H / 2][W / 2]."""
    image = np.asarray(image, dtype=F)
    W, H = image.shape[:2]
    assert image.shape == (W, H, 3) and W % 2 == 0 and H % 2 == 0 and W > 0 and H > 0
    vals, spans = prequant(image, format, matrix, range, siting)
    out = []
    for plane, (s, (lo, hi)) in enumerate(zip(vals, spans)):
        q = quantise(s, lo, hi, mode, seed, phase, plane)
        assert q.min() >= int(lo) and q.max() <= int(hi)
        out.append(q)
    return tuple(out)


def assemble(y, cb, cr, format):
    """Codes to the frame's bytes."""
    dt = np.uint16 if bits(format) == 10 else np.uint8
    shift = 6 if format == "p010" else 0
    y, cb, cr = [(np.asarray(p).astype(np.int64) << shift).astype(dt) for p in (y, cb, cr)]
    if format in ("nv12", "p010"):
        parts = [y.ravel(), np.stack([cb, cr], axis=-1).ravel()]
    else:
        parts = [y.ravel(), cb.ravel(), cr.ravel()]
    return np.concatenate(parts).astype("<u2" if dt is np.uint16 else np.uint8).view(np.uint8)


def pack(image, format="nv12", matrix="bt709", range="limited", siting="left", mode="round", seed=0, phase=0):
    return assemble(*codes(image, format, matrix, range, siting, mode, seed, phase), format=format)


def planes(frame, W, H, format):
    """The frame's (Y, Cb, Cr) codes as int64 arrays (P010's shift undone), whatever the layout."""
    flat = np.asarray(frame).reshape(-1).view(np.uint8)
    if bits(format) == 10:
        flat = flat.view("<u2")
    assert flat.size == W * H * 3 // 2, (flat.size, W, H)
    flat = flat.astype(np.int64)
    y = flat[:W * H].reshape(H, W)
    if format in ("nv12", "p010"):
        c = flat[W * H:].reshape(H // 2, W // 2, 2)
        cb, cr = c[..., 0], c[..., 1]
    else:
        n = (W // 2) * (H // 2)
        cb, cr = flat[W * H:W * H + n].reshape(H // 2, W // 2), flat[W * H + n:].reshape(H // 2, W // 2)
    if format == "p010":
        assert not ((y & 63).any() or (cb & 63).any() or (cr & 63).any())
        y, cb, cr = y >> 6, cb >> 6, cr >> 6
    return y, cb, cr
