"""A numpy float32 restatement of the history reprojection of the display path (include/digital_earth_history.h): the camera basis, the
pixel's world point, its projection into the history's camera, the four unclamped bilinear taps with their validity, the blend and the candidate.  It
shares no code with csrc/.  Every step is f32 `+ - * /`, sqrt, floor and compares in the order the design states, so the device must give the same
bits.  Arrays are (W, H, k) in fetch_hdr's layout: axis 0 is x (u), axis 1 is y (v)."""
import numpy as np

DEFAULTS = dict(max_history=32.0, depth_tolerance=0.02)
FLT_MAX = np.finfo(np.float32).max
F = np.float32


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _normalized(a):
    """Vector.normalized() in IEEE f32: a * (1 / sqrt(dot(a, a))), one reciprocal shared by the three components."""
    inv = F(1.0) / np.sqrt(_dot(a, a))
    return [a[0] * inv, a[1] * inv, a[2] * inv]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def camera(params, W, H):
    """The camera of a de_params (anything with camera_pos, look_at, up, fov, aspect_scale) on a W x H image: setup_kernel's expression."""
    cam = [F(params.camera_pos[k]) for k in range(3)]
    look = [F(params.look_at[k]) for k in range(3)]
    up = [F(params.up[k]) for k in range(3)]
    d = _normalized([look[k] - cam[k] for k in range(3)])
    du = _normalized(_cross(d, up))
    dv = _normalized(_cross(du, d))
    return dict(cam=cam, d=d, du=du, dv=dv, fov=F(params.fov), ar=F(np.float64(W) / np.float64(H)), asc=F(params.aspect_scale))


def rays(cam, W, H):
    """The IEEE-normalised ray through every pixel centre: three (W, H) arrays."""
    u = np.arange(W, dtype=np.float32)[:, None] + np.zeros((1, H), np.float32)
    v = np.arange(H, dtype=np.float32)[None, :] + np.zeros((W, 1), np.float32)
    Hf, fov = F(H), cam["fov"]
    fu = (F(2.0) * fov * (u + F(0.5)) / Hf - fov * cam["ar"] - F(1e-5)) * cam["asc"]
    fv = F(2.0) * fov * (v + F(0.5)) / Hf - fov - F(1e-5)
    a = [(cam["d"][k] + fu * cam["du"][k]) + fv * cam["dv"][k] for k in range(3)]
    return _normalized(a)


def project(q, hcam, W, H):
    """q (three arrays) into the history's camera: z, and the continuous pixel coordinates (xo, yo) in the centre convention."""
    Hf = F(H)
    z = _dot(q, hcam["d"])
    gu, gv = _dot(q, hcam["du"]) / z, _dot(q, hcam["dv"]) / z
    xo = ((gu / hcam["asc"] + F(1e-5)) + hcam["fov"] * hcam["ar"]) * Hf / (F(2.0) * hcam["fov"]) - F(0.5)
    yo = ((gv + F(1e-5)) + hcam["fov"]) * Hf / (F(2.0) * hcam["fov"]) - F(0.5)
    return z, xo, yo


def reproject(dist, cam, hist_c, hist_d, hcam, max_history=32.0, depth_tolerance=0.02):
    """Steps 2 - 6 for every pixel.  Returns dict(have, h (W, H, 3), w, B, xo, yo, z, r, x0, y0, valid (4, W, H): the taps (x0 + (k & 1), y0 + (k >> 1)))."""
    dist = np.asarray(dist, np.float32)
    hist_c, hist_d = np.asarray(hist_c, np.float32), np.asarray(hist_d, np.float32)
    W, H = dist.shape
    with np.errstate(all="ignore"):
        dr = rays(cam, W, H)
        land = dist > 0
        s = -_dot(cam["cam"], dr)
        t = np.where(land, dist, s)
        # the camera's step first: (cam + dir t) - cam_h would round the world point at planet scale and keep that error however short the ray
        step = [cam["cam"][k] - hcam["cam"][k] for k in range(3)]
        at_infinity = ~land & ~(s > 0)
        q = [np.where(at_infinity, dr[k], step[k] + dr[k] * t) for k in range(3)]
        z, xo, yo = project(q, hcam, W, H)
        ok = (z > 0) & (xo >= F(-1.0)) & (xo < F(W)) & (yo >= F(-1.0)) & (yo < F(H))
        xs, ys = np.where(ok, xo, F(0)), np.where(ok, yo, F(0))
        fx, fy = np.floor(xs), np.floor(ys)
        bx, by = xs - fx, ys - fy
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        r = np.sqrt(_dot(q, q))
        tol = F(depth_tolerance) * r
        zero = np.zeros((W, H), np.float32)
        terms, valids = [], []
        for k in range(4):
            xi, yi = x0 + (k & 1), y0 + (k >> 1)
            inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            c = hist_c[np.clip(xi, 0, W - 1), np.clip(yi, 0, H - 1)]
            hd = hist_d[np.clip(xi, 0, W - 1), np.clip(yi, 0, H - 1)]
            finite = (np.abs(c[..., 0]) <= FLT_MAX) & (np.abs(c[..., 1]) <= FLT_MAX) & (np.abs(c[..., 2]) <= FLT_MAX)
            surface = np.where(land, (hd > 0) & (np.abs(hd - r) <= tol), hd == 0)
            valid = ok & inside & (c[..., 3] > 0) & finite & surface
            valids.append(valid)
            b = ((bx if k & 1 else F(1.0) - bx) * (by if k >> 1 else F(1.0) - by)).astype(np.float32)
            # an invalid tap contributes +0 to every sum
            terms.append([np.where(valid, b, F(0))] + [np.where(valid, b * c[..., ch], F(0)) for ch in (3, 0, 1, 2)])
        # the two taps of a row first, then the two rows
        B, Ws, h0, h1, h2 = [(terms[0][i] + terms[1][i]) + (terms[2][i] + terms[3][i]) for i in range(5)]
        hs = [h0, h1, h2]
        have = B > 0
        h = np.stack([hs[ch] / B for ch in range(3)], axis=-1)
        wm = Ws / B
        mh = F(max_history)
        w = np.where(wm < mh, wm, mh) * B
    return dict(have=have, h=np.where(have[..., None], h, F(0)).astype(np.float32), w=np.where(have, w, F(0)).astype(np.float32), B=B, xo=xo, yo=yo, z=z, r=r, x0=x0, y0=y0, valid=np.stack(valids))


def blend(m, n, dist, cam, hist_c=None, hist_d=None, hcam=None, max_history=32.0, depth_tolerance=0.02, details=False):
    """Steps 1 - 7 from the mean m (W, H, 3), the per-pixel sample counts n (a scalar or (W, H)), the current distance guide and camera, and the
    history (hist_c (W, H, 4) = rgb + weight, hist_d (W, H), its camera; None: no history yet).  Returns (W, H, 4): the blended mean and Wout —
    which, with a copy of dist and the current camera, is the next history candidate."""
    m = np.asarray(m, np.float32)
    W, H = m.shape[:2]
    n = np.broadcast_to(np.asarray(n), (W, H))
    nf = n.astype(np.float32)
    out = np.concatenate([m, nf[..., None]], axis=-1).astype(np.float32)
    if hist_c is None:
        return (out, None) if details else out
    rp = reproject(dist, cam, hist_c, hist_d, hcam, max_history, depth_tolerance)
    with np.errstate(all="ignore"):
        h, w = rp["h"], rp["w"]
        wsum = nf + w
        mixed = (m * nf[..., None] + h * w[..., None]) / wsum[..., None]
        first = np.concatenate([h, w[..., None]], axis=-1)
        later = np.concatenate([mixed, wsum[..., None]], axis=-1)
        out = np.where(rp["have"][..., None], np.where((n == 0)[..., None], first, later), out).astype(np.float32)
    return (out, rp) if details else out


def mean_of(sums, samples):
    """Step 1: the display's own division, f32 sum / f32 count.  samples: a scalar or (W, H) per-pixel counts."""
    s = np.asarray(sums, dtype=np.float32)
    c = np.asarray(samples).astype(np.float32)
    if c.ndim == 2:
        c = c[..., None]
    with np.errstate(all="ignore"):
        return (s / c).astype(np.float32)
