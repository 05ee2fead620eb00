"""The history reprojection of the display path (include/digital_earth_history.h) stated in float64 from DESIGN.md §13 steps 2 - 7, independently of
tests/history_ref.py and of csrc/: it takes the same f32 inputs (the camera-basis dicts of history_ref.camera, dist, hist_c, hist_d, max_history,
depth_tolerance, m, n), widens them and does everything else in float64 — where the geometry is exact to about 1e-9 m at planet scale, so the order of
its sums does not matter.  Arrays are (W, H, k) in fetch_hdr's layout: axis 0 is x (u), axis 1 is y (v).

Besides the model's quantities it returns, per pixel, where an f32 evaluation of the same model is ILL-CONDITIONED: a decision of the model (a floor, a
compare) sits within the f32 evaluation's error of its threshold, so either answer is a correct rounding.  The error budgets are counted in units of one
f32 rounding, 2^-24 of the quantity's own size:

    position   n_pos S,  S = 2^-24 max(W, H, H / (2 fov_h)) pixels: one rounding of a quantity of image size, or of gu scaled to pixels
    r, z       n_len 2^-24 (|cam - cam_h| + |t|): every term of q = (cam - cam_h) + dir t is rounded relative to itself (at infinity q = dir: 2^-24 n_len)
    s          n_s 2^-24 |cam|: s = -dot(cam, dir) is a sum of products of planet size whatever its own size
    B          4 (2 n_pos S + 3 2^-24) + 3 2^-24: four weights (1 - bx | bx)(1 - by | by), each moved by the position error of both axes, and the sum

n_pos, n_len and n_s are the caller's (tests/history_cases.py counts them from the model's operations)."""
import numpy as np

EPS = 2.0 ** -24


def _v(a):
    return [np.float64(a[k]) for k in range(3)]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _unit(a):
    n = np.sqrt(_dot(a, a))
    return [a[k] / n for k in range(3)]


def rays(cam, W, H):
    """Step 2: the unit ray through every pixel centre, three (W, H) float64 arrays."""
    u = np.arange(W, dtype=np.float64)[:, None] + np.zeros((1, H))
    v = np.arange(H, dtype=np.float64)[None, :] + np.zeros((W, 1))
    fov, ar, asc = np.float64(cam["fov"]), np.float64(cam["ar"]), np.float64(cam["asc"])
    fu = (2.0 * fov * (u + 0.5) / H - fov * ar - 1e-5) * asc
    fv = 2.0 * fov * (v + 0.5) / H - fov - 1e-5
    d, du, dv = _v(cam["d"]), _v(cam["du"]), _v(cam["dv"])
    return _unit([d[k] + fu * du[k] + fv * dv[k] for k in range(3)])


def pixel_scale(hcam, W, H):
    """S: one f32 rounding of a quantity of image size, or of gu scaled to pixels, in pixels."""
    return EPS * max(W, H, H / (2.0 * float(hcam["fov"])))


def history(cam, dist, hist_c, hist_d, hcam, max_history, depth_tolerance, m, n, n_pos, n_len, n_s):
    """Steps 2 - 7.  Returns a dict: land, s, xo, yo, z, r, x0, y0, valid (4, W, H: the taps (x0 + (k & 1), y0 + (k >> 1))), full (every tap that any
    floor() within the position budget would read is valid), B, h (W, H, 3), w, have,
    out (W, H, 3), Wout; the budgets pos, len (W, H), s_bound, B_bound; inside (the projection lies in -1 <= xo < W, -1 <= yo < H by more than pos);
    and ill: a dict of (W, H) masks grid, depth, z, s, B and their union any."""
    dist = np.asarray(dist, np.float32).astype(np.float64)
    hist_c, hist_d = np.asarray(hist_c, np.float32).astype(np.float64), np.asarray(hist_d, np.float32).astype(np.float64)
    m = np.asarray(m, np.float32).astype(np.float64)
    W, H = dist.shape
    n = np.broadcast_to(np.asarray(n), (W, H)).astype(np.float64)
    mh, tolf = np.float64(np.float32(max_history)), np.float64(np.float32(depth_tolerance))
    c, ch = _v(cam["cam"]), _v(hcam["cam"])
    with np.errstate(all="ignore"):
        # steps 2 - 3: the pixel's world point relative to the history's camera
        dr = rays(cam, W, H)
        land = dist > 0
        s = -_dot(c, dr)
        at_infinity = ~land & ~(s > 0)
        t = np.where(land, dist, s)
        step = [c[k] - ch[k] for k in range(3)]
        q = [np.where(at_infinity, dr[k], step[k] + dr[k] * t) for k in range(3)]
        # step 4: its projection
        fov, ar, asc = np.float64(hcam["fov"]), np.float64(hcam["ar"]), np.float64(hcam["asc"])
        z = _dot(q, _v(hcam["d"]))
        gu, gv = _dot(q, _v(hcam["du"])) / z, _dot(q, _v(hcam["dv"])) / z
        xo = (gu / asc + 1e-5 + fov * ar) * H / (2.0 * fov) - 0.5
        yo = (gv + 1e-5 + fov) * H / (2.0 * fov) - 0.5
        ok = (z > 0) & (xo >= -1.0) & (xo < W) & (yo >= -1.0) & (yo < H)
        xs, ys = np.where(ok, xo, 0.0), np.where(ok, yo, 0.0)
        fx, fy = np.floor(xs), np.floor(ys)
        bx, by = xs - fx, ys - fy
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        r = np.sqrt(_dot(q, q))
        # the budgets
        pos = n_pos * pixel_scale(hcam, W, H)
        length = np.where(at_infinity, 1.0, np.sqrt(_dot(step, step)) + np.abs(t))
        len_bound = n_len * EPS * length
        s_bound = n_s * EPS * np.sqrt(_dot(c, c))
        B_bound = 4.0 * (2.0 * pos + 3.0 * EPS) + 3.0 * EPS
        # step 5: the taps
        def tap(xi, yi):
            """(inside, its colour and weight, valid but for the range test, |Hd - r| within the budgets of depth_tolerance r) of history pixel (xi, yi)."""
            inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            cc = hist_c[np.clip(xi, 0, W - 1), np.clip(yi, 0, H - 1)]
            hd = hist_d[np.clip(xi, 0, W - 1), np.clip(yi, 0, H - 1)]
            finite = np.isfinite(cc[..., :3]).all(axis=-1)
            off = np.abs(hd - r)
            surface = np.where(land, (hd > 0) & (off <= tolf * r), hd == 0)
            # |Hd - r| against depth_tolerance r: r's own budget on both sides, and the two f32 roundings of the compare's operands
            near = inside & land & (hd > 0) & (np.abs(off - tolf * r) <= len_bound * (1.0 + tolf) + 2.0 * EPS * (off + tolf * r))
            return inside & (cc[..., 3] > 0) & finite & surface, near
        valid, weights, near_tolerance = [], [], np.zeros((W, H), bool)
        for k in range(4):
            good, near = tap(x0 + (k & 1), y0 + (k >> 1))
            valid.append(ok & good)
            weights.append((bx if k & 1 else 1.0 - bx) * (by if k >> 1 else 1.0 - by))
            near_tolerance |= ok & near
        # every tap of every floor() within the position budget is valid and away from the tolerance: off the grid these are the four taps, on it a
        # row or a column more (the still camera: the 3 x 3 pixels about the pixel itself)
        xl, xh = np.floor(np.where(ok, xo - pos, 0.0)).astype(np.int64), np.floor(np.where(ok, xo + pos, 0.0)).astype(np.int64) + 1
        yl, yh = np.floor(np.where(ok, yo - pos, 0.0)).astype(np.int64), np.floor(np.where(ok, yo + pos, 0.0)).astype(np.int64) + 1
        full = ok.copy()
        for i in range(3):
            for j in range(3):
                good, near = tap(xl + i, yl + j)
                full &= (good & ~near) | (xl + i > xh) | (yl + j > yh)
        # step 6
        B = sum(np.where(valid[k], weights[k], 0.0) for k in range(4))
        have = B > 0
        h = np.stack([sum(np.where(valid[k], weights[k] * hist_c[np.clip(x0 + (k & 1), 0, W - 1), np.clip(y0 + (k >> 1), 0, H - 1), i], 0.0) for k in range(4)) / B
                      for i in range(3)], axis=-1)
        Ws = sum(np.where(valid[k], weights[k] * hist_c[np.clip(x0 + (k & 1), 0, W - 1), np.clip(y0 + (k >> 1), 0, H - 1), 3], 0.0) for k in range(4))
        w = np.minimum(Ws / B, mh) * B
        h, w = np.where(have[..., None], h, 0.0), np.where(have, w, 0.0)
        # step 7
        Wout = np.where(have, np.where(n == 0, w, n + w), n)
        mixed = (m * n[..., None] + h * w[..., None]) / (n + w)[..., None]
        out = np.where(have[..., None], np.where((n == 0)[..., None], h, mixed), m)
        # where an f32 evaluation may decide otherwise
        reach = (z > 0) & (xo >= -1.0 - pos) & (xo <= W + pos) & (yo >= -1.0 - pos) & (yo <= H + pos)      # a tap may be read at all
        grid = reach & ((np.abs(xo - np.rint(xo)) <= pos) | (np.abs(yo - np.rint(yo)) <= pos))            # an integer: a floor, or one of the limits -1, W, H
        ill = dict(grid=grid, depth=near_tolerance, z=np.abs(z) <= len_bound, s=~land & (np.abs(s) <= s_bound),
                   B=np.any(valid, axis=0) & (B <= B_bound))
        ill["any"] = ill["grid"] | ill["depth"] | ill["z"] | ill["s"] | ill["B"]
        inside = (z > 0) & (xo >= -1.0 + pos) & (xo < W - pos) & (yo >= -1.0 + pos) & (yo < H - pos)
    return dict(land=land, s=s, at_infinity=at_infinity, xo=xo, yo=yo, z=z, r=r, x0=x0, y0=y0, valid=np.stack(valid), full=full, B=B, h=h, w=w, have=have, out=out,
                Wout=Wout, gu=gu, gv=gv, step=np.sqrt(_dot(step, step)), pos=pos, len=len_bound, s_bound=s_bound, B_bound=B_bound, inside=inside, ill=ill)
