"""The low-camera cases of the history reprojection's float64 tests (tests/test_history_f64.py on the CPU, tests/test_gpu_history.py on the device,
tools/history_host_check.py on the host): cameras from 2 m above a smooth sphere to the suite's 21 000 km one, the five history cameras, the sphere's
distance guides, a smooth history, and the error budgets the comparisons use, counted in f32 roundings.  No GPU and no csrc/ code.

The budgets (one rounding = 2^-24 of the quantity's own size):

  N_POS, position in units of S = 2^-24 max(W, H, H / (2 fov_h)) px.  Roundings of steps 2 - 4 on the way to xo:
      fu 6 (the product with u + 0.5, / H, fov aspect_ratio, two differences, aspect_scale), fv 4, (d + fu du) + fv dv 4 x 3,
      normalized_ieee 10 (dot 5, sqrt, reciprocal, three products), cam - cam_h 3, dir t 3, their sum 3, z 5, dot(q, du_h) 5, / z 1,
      xo 7 (/ aspect_scale, + 1e-5, fov aspect_ratio, +, H, /, - 0.5): 59 (yo: 57).  Each moves xo by about one S or less: a rounding of q's terms is
      relative to a length no larger than z / cos, which gu = dot / z turns into 2^-24 H / (2 fov_h) px, and a rounding of xo's own chain is relative
      to a quantity of image size.  Measured over the whole sweep of tests/test_history_f64.py against tests/history_f64.py: 4.1 S on land, 3.5 S at
      the tangent point beyond its parallax, 4.2 S at infinity (MEASURED_POS = 4.3 holds them); N_POS = max(59, 4 x 4.3) = 59.
  N_LEN, r and z in units of 2^-24 (|cam - cam_h| + |t|): dir's 32 (fu, fv, the sum, the normalisation), cam - cam_h 3, dir t 3, their sum 3, the dot 5,
      r's sqrt 1: 47.  Measured on land: 4.15 (MEASURED_LEN = 4.2); N_LEN = max(47, 4 x 4.2) = 47.
  N_S, s = -dot(cam, dir) in units of 2^-24 |cam|: dir's 32 and the dot's 5: 37.
  K_BLEND, out in units of 2^-24 max(|m|, |h|), steps 6 - 7: a tap's weight 3 (1 - bx, 1 - by, their product) and its product with the colour 1, the
      two levels of the sum 2, B's own 3 + 2, / B 1: 12 for h; the same 12 for sum b Wh, / B, the product with B: 14 for w, which moves out by at most
      |h - m| n dw / (n + w)^2 <= max(|m|, |h|) (dw / w) / 2: 7; m n, h w, their sum, n + w, the quotient: 5.  24, and 5 % more because a rounding of
      a tap is relative to that tap's colour, which the smooth history keeps within 5 % of h: 26."""
from types import SimpleNamespace

import numpy as np

import history_f64 as h64
import history_ref as hr

F = np.float32
RADIUS = 6371e3
COUNT_POS, COUNT_LEN, COUNT_S, K_BLEND = 59, 47, 37, 26
MEASURED_POS, MEASURED_LEN = 4.3, 4.2          # the worst of the corrected restatement over the sweep, in S and in 2^-24 (|cam - cam_h| + |t|)
N_POS = max(COUNT_POS, 4.0 * MEASURED_POS)
N_LEN = max(COUNT_LEN, 4.0 * MEASURED_LEN)
N_S = COUNT_S

SIZES = [(16, 8), (80, 56)]
# name -> (the camera's direction from the planet's centre, its altitude).  Near the ground the direction is close to +z, so that x and y stay small
# enough for f32 to hold a step of 1 % of 2 m; "21 000 km" is the camera of tests/test_gpu_history.py; "100 m, oblique" has all three coordinates
# of planet size, so that nothing rests on the alignment of the others (there the former expression is off in every axis).
ALTITUDES = {"2 m": ((0.003, 0.002, 1.0), 2.0), "100 m": ((0.003, 0.002, 1.0), 100.0), "10 km": ((0.003, 0.002, 1.0), 1e4),
             "400 km": ((0.003, 0.002, 1.0), 4e5), "21 000 km": ((-1.0, 0.0, 1.0), float(np.hypot(15e6, 15e6)) - RADIUS),
             "100 m, oblique": ((0.48, 0.6, 0.64), 100.0)}
FOVS = [0.4, 0.05]
VIEWS = ["horizon", "down", "up"]
HISTORY_CAMERAS = ["identical", "yaw 1.5 px", "step 1 %", "step 30 % zoom 1.2", "turned around"]
WEIGHTS = [0.5, 9.0, 100.0]


def params(pos, look, fov):
    return SimpleNamespace(camera_pos=[float(F(x)) for x in pos], look_at=[float(F(x)) for x in look], up=[0.0, 1.0, 0.0], fov=float(F(fov)), aspect_scale=1.0)


def _turned(o, yaw, pitch):
    """o turned about the up axis by `yaw` and towards it by `pitch`.  A pure yaw leaves yo on the pixel grid and a pure step leaves the pixels at
    infinity there, where floor() is anyone's; the fractions of a pixel added to either keep every case but "identical" off the grid."""
    o = np.array([np.cos(yaw) * o[0] + np.sin(yaw) * o[2], o[1], -np.sin(yaw) * o[0] + np.cos(yaw) * o[2]])
    return np.cos(pitch) * o + np.sin(pitch) * np.linalg.norm(o) * np.array([0.0, 1.0, 0.0])


def camera_pair(altitude, fov, view, history, H):
    """(params of the current camera, params of the history's) for one case.  `up` is y; the frame (e1, e2, up-from-the-ground) is orthonormal with e2
    close to y, so that e2 is sideways for all three views."""
    direction, alt = ALTITUDES[altitude]
    nrm = np.array(direction, np.float64) / np.linalg.norm(direction)
    pos = nrm * (RADIUS + alt)
    e1 = np.cross([0.0, 1.0, 0.0], nrm)
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    dip = np.arccos(RADIUS / (RADIUS + alt))                      # the limb runs through the middle of the image: land, limb and sky
    # down is off the vertical by a fraction of a pixel: on it the image is four-fold symmetric, and what one pixel meets (a neighbour exactly at the
    # depth tolerance, at 16x8 and fov 0.4) four do
    off = 2.0 * fov / H
    axis = {"horizon": np.cos(dip) * e1 - np.sin(dip) * nrm, "down": -nrm + 0.37 * off * e1 + 0.21 * off * e2, "up": nrm}[view]
    reach = max(1e5, 10.0 * alt)
    look = pos + axis * reach
    hpos, hlook, hfov = pos, look, fov
    if history == "yaw 1.5 px":
        hlook = pos + _turned(look - pos, 1.5 * 2.0 * fov / H, 0.37 * 2.0 * fov / H)
    elif history == "step 1 %":
        move = 0.01 * alt * (0.36 * e1 + 0.8 * e2 + 0.48 * nrm)
        hpos, hlook = pos + move, pos + move + _turned(look - pos, 0.43 * 2.0 * fov / H, 0.27 * 2.0 * fov / H)
    elif history == "step 30 % zoom 1.2":
        move = 0.3 * alt * (0.6 * e1 + 0.64 * e2 + 0.48 * nrm)
        hpos, hlook, hfov = pos + move, pos + move + _turned(look - pos, 0.21 * 2.0 * fov / H, 0.17 * 2.0 * fov / H), fov * 1.2
    elif history == "turned around":
        hlook = 2.0 * pos - look
    else:
        assert history == "identical"
    return params(pos, look, fov), params(hpos, hlook, hfov)


def sphere_distance(cam, W, H):
    """The float64 distance from the camera to the smooth sphere along every pixel's ray, rounded to f32 (0 where the ray misses)."""
    d = h64.rays(cam, W, H)
    o = [np.float64(x) for x in cam["cam"]]
    b = sum(d[k] * o[k] for k in range(3))
    oo = np.sqrt(sum(o[k] * o[k] for k in range(3)))
    c = (oo - RADIUS) * (oo + RADIUS)
    disc = b * b - c
    t = np.where((disc > 0) & (b < 0), c / (-b + np.sqrt(np.maximum(disc, 0.0))), 0.0)
    return np.where(t > 0, t, 0.0).astype(np.float32)


# The smooth history: per channel a level, a linear ramp in x and y and one low-frequency sinusoid.  Between neighbouring pixels it changes by at most
# GX in x and GY in y, and a bilinear interpolation of its samples has no steeper slope: a position error of e px in both axes moves h by (GX + GY) e.
_RAMP_X, _RAMP_Y, _AMP, _KX, _KY = 0.004, -0.003, 0.08, 0.09, 0.06
GRADIENT = (_RAMP_X + _AMP * _KX) + (abs(_RAMP_Y) + _AMP * _KY)


def smooth_history(W, H, weight):
    x = np.arange(W, dtype=np.float64)[:, None] + np.zeros((1, H))
    y = np.arange(H, dtype=np.float64)[None, :] + np.zeros((W, 1))
    c = [1.6 + 0.3 * ch + _RAMP_X * x + _RAMP_Y * y + _AMP * np.sin(_KX * x + _KY * y + 0.7 * ch) for ch in range(3)]
    return np.stack(c + [np.full((W, H), weight)], axis=-1).astype(np.float32)


def smooth_mean(W, H):
    x = np.arange(W, dtype=np.float64)[:, None] + np.zeros((1, H))
    y = np.arange(H, dtype=np.float64)[None, :] + np.zeros((W, 1))
    return np.stack([0.9 + 0.2 * ch + 0.3 * np.cos(0.05 * x - 0.08 * y + ch) for ch in range(3)], axis=-1).astype(np.float32)


def counts(W, H):
    """n in {0, 1, 7}, every value in every 2 x 2 block of pixels."""
    x = np.arange(W)[:, None] + np.zeros((1, H), np.int64)
    y = np.arange(H)[None, :] + np.zeros((W, 1), np.int64)
    return np.array([0, 1, 7, 1], np.int32)[(x & 1) + 2 * (y & 1)]


_CASES = {}


def case(size, altitude, fov, view, history):
    """One case, made once and never changed: the two de_params-like cameras (p, hp), their f32 bases (cam, hcam), dist, hist_d, hist (W, H, 4), m, n,
    and f64: the float64 statement with the budgets above."""
    key = (size, altitude, fov, view, history)
    if key not in _CASES:
        W, H = size
        p, hp = camera_pair(altitude, fov, view, history, H)
        cam, hcam = hr.camera(p, W, H), hr.camera(hp, W, H)
        index = [list(ALTITUDES).index(altitude), FOVS.index(fov), VIEWS.index(view), HISTORY_CAMERAS.index(history)]
        x = dict(p=p, hp=hp, cam=cam, hcam=hcam, dist=sphere_distance(cam, W, H), hist_d=sphere_distance(hcam, W, H),
                 hist=smooth_history(W, H, WEIGHTS[sum(index) % 3]), m=smooth_mean(W, H), n=counts(W, H))
        x["f64"] = h64.history(cam, x["dist"], x["hist"], x["hist_d"], hcam, hr.DEFAULTS["max_history"], hr.DEFAULTS["depth_tolerance"], x["m"], x["n"],
                               N_POS, N_LEN, N_S)
        for a in x.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[key] = x
    return _CASES[key]


def sky_parallax(f):
    """What s's own rounding adds to the position of a tangent-point pixel (not land, s > 0), in pixels.  s = -dot(cam, dir) is off by ds <= N_S 2^-24
    |cam| whatever its size, which moves q = (cam - cam_h) + dir s along dir by ds.  With dir = (q - step) / s (step = cam - cam_h), the change of
    gu = dot(q, du_h) / z is  ds / s [(q.du_h - step.du_h) / z - (q.du_h)(q.d_h - step.d_h) / z^2] = ds / (s z) [gu step.d_h - step.du_h]:  the terms in
    q alone cancel (a point moving along the ray through the history's own eye does not move in its image), and what is left is at most
    ds |step| sqrt(1 + gu^2) / (s z) — times H / (2 fov_h) in pixels; aspect_scale_h is 1 here.  The same in v.  With no step there is none."""
    with np.errstate(all="ignore"):
        scale = f["pos"] / N_POS / h64.EPS                                     # max(W, H, H / (2 fov_h)) >= H / (2 fov_h)
        g = np.sqrt(1.0 + np.maximum(f["gu"] ** 2, f["gv"] ** 2))
        return np.where(f["step"] > 0, f["s_bound"] * f["step"] * g / (np.abs(f["s"]) * np.abs(f["z"])) * scale, 0.0)


def blend_bound(x, gradient=None):
    """|out_f32 - out_f64| <= G N S + k 2^-24 max(|m|, |h|) where all four taps are valid.  Where a tap is missing (an image border, a depth edge) h is
    sum b c / B over the valid ones and w = min(Wh, max_history) B move with B too: dh/dbx = sum (db/dbx)(c - h) / B with sum |db/dbx| <= 2 and
    |c - h| <= G, so h moves by at most 4 G N S / B; B by at most 4 N S, which moves out by |h - m| n dw / (n + w)^2 <= |h - m| dB / (4 B):
    (4 G + |h - m|) N S / B there.  "All four" is f["full"]: on the grid (the still camera's pixels) floor() may go either way, so the taps of both
    choices count — there the plain bound holds where the 3 x 3 history pixels about the pixel are valid, and the wider one only where one of them is
    invalid or outside the image."""
    f = x["f64"]
    G = GRADIENT if gradient is None else gradient
    m = np.asarray(x["m"]).astype(np.float64)
    h = f["h"]
    full = f["full"]
    with np.errstate(all="ignore"):
        partial = (4.0 * G + np.abs(h - m)) / np.maximum(f["B"], 1e-300)[..., None]
    geometric = np.where(full[..., None], G, partial) * f["pos"]
    return np.where(f["have"][..., None], geometric + K_BLEND * h64.EPS * np.maximum(np.abs(m), np.abs(h)), 0.0)
