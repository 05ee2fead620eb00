"""Properties of the numpy float32 restatement of the history reprojection (tests/history_ref.py), without a GPU: a still camera maps
every pixel onto itself, constants stay constants, a depth step uncovers exactly its band, a camera turned around finds nothing, a long frame
outweighs its history, and a zoom keeps the optical axis."""
from types import SimpleNamespace

import numpy as np

import history_ref as hr

W, H = 80, 56
F = np.float32


def params(pos=(-15000000.0, 0.0, 15000000.0), look=(0.0, 0.0, 0.0), fov=float(np.radians(27.0) * 0.5), aspect_scale=1.0):
    return SimpleNamespace(camera_pos=[float(F(x)) for x in pos], look_at=[float(F(x)) for x in look], up=[0.0, 1.0, 0.0], fov=float(F(fov)),
                           aspect_scale=float(F(aspect_scale)))


def f64(v):
    return np.array([np.float64(x) for x in v])


def sphere_distance(cam, radius=6371e3):
    """First hit of every pixel's ray with a sphere at the origin, in float64 (0 where it misses): a synthetic land distance guide."""
    d = np.stack([x.astype(np.float64) for x in hr.rays(cam, W, H)], axis=-1)
    o = f64(cam["cam"])
    b = d @ o
    disc = b * b - (o @ o - radius * radius)
    t = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0.0)), 0.0)
    return np.where(t > 0, t, 0.0).astype(np.float32)


def yawed(p, pixels):
    """p with its look-at point turned about the up axis by `pixels` pixels of the image."""
    cam, look = np.array(p.camera_pos), np.array(p.look_at)
    a = pixels * 2.0 * p.fov / H
    o = look - cam
    c, s = np.cos(a), np.sin(a)
    o = np.array([c * o[0] + s * o[2], o[1], -s * o[0] + c * o[2]])
    return params(pos=cam, look=cam + o, fov=p.fov, aspect_scale=p.aspect_scale)


def test_a_still_camera_maps_every_pixel_onto_itself():
    cam = hr.camera(params(), W, H)
    dist = sphere_distance(cam)
    assert 0.2 < (dist > 0).mean() < 1.0                                  # land, limb and sky
    hist_c = np.ones((W, H, 4), np.float32)
    rp = hr.reproject(dist, cam, hist_c, dist, cam)
    u = np.arange(W)[:, None] + np.zeros((1, H))
    v = np.arange(H)[None, :] + np.zeros((W, 1))
    assert np.abs(rp["xo"] - u).max() < 1e-3 and np.abs(rp["yo"] - v).max() < 1e-3
    assert rp["have"].all()
    assert np.abs(rp["B"][1:-1, 1:-1] - 1.0).max() < 1e-3


def test_a_constant_stays_a_constant():
    p = params()
    cam, hcam = hr.camera(yawed(p, 1.37), W, H), hr.camera(p, W, H)
    dist, hist_d = sphere_distance(cam), sphere_distance(hcam)
    c = F(0.4)
    hist_c = np.concatenate([np.full((W, H, 3), c), np.full((W, H, 1), F(9.0))], axis=-1).astype(np.float32)
    m = np.full((W, H, 3), c, np.float32)
    for n in (1, 7):
        out, rp = hr.blend(m, n, dist, cam, hist_c, hist_d, hcam, details=True)
        assert rp["have"].mean() > 0.9
        ulp = np.spacing(c)
        assert np.abs(out[..., :3].astype(np.float64) - np.float64(c)).max() <= 2 * ulp
        assert (out[..., 3][rp["have"]] > n).all() and (out[..., 3][~rp["have"]] == n).all()


def test_a_depth_step_uncovers_exactly_its_band():
    """The history saw a foreground (distance 1e7 m) on the left half of the image and a background (2e7 m) on the right; both are spheres about the
    history's camera.  The camera then steps 1000 km to its right: the foreground's edge moves left by about six pixels more than the background."""
    ph = params()
    hcam = hr.camera(ph, W, H)
    near, far, step = 1e7, 2e7, 1e6
    c_h, du_h = f64(hcam["cam"]), f64(hcam["du"])
    pos = c_h + step * du_h
    pc = params(pos=pos, look=pos + f64(hcam["d"]) * 1e7)
    cam = hr.camera(pc, W, H)
    hist_d = np.where(np.arange(W)[:, None] < W // 2, F(near), F(far)) + np.zeros((1, H), np.float32)
    # the same scene from the new camera, in float64
    d = np.stack([x.astype(np.float64) for x in hr.rays(cam, W, H)], axis=-1)
    o = f64(cam["cam"]) - c_h
    b = d @ o

    def hit(radius):
        return -b + np.sqrt(b * b - (o @ o - radius * radius))

    def history_x(t):
        q = o + d * t[..., None]
        z = q @ f64(hcam["d"])
        fu = (q @ du_h) / z
        fov, ar = np.float64(hcam["fov"]), np.float64(hcam["ar"])
        fv = (q @ f64(hcam["dv"])) / z
        return (fu + 1e-5 + fov * ar) * H / (2 * fov) - 0.5, (fv + 1e-5 + fov) * H / (2 * fov) - 0.5
    x_near, _ = history_x(hit(near))
    foreground = x_near < W // 2 - 0.5
    dist = np.where(foreground, hit(near), hit(far)).astype(np.float32)
    x_h, y_h = history_x(dist.astype(np.float64))
    interior = (x_h >= 0) & (x_h <= W - 1) & (y_h >= 0) & (y_h <= H - 1)
    assert np.abs(x_h[~foreground] - (W // 2 - 1)).min() > 1e-3           # no background point lands on the column where the band ends: its edge is unambiguous
    band = ~foreground & (np.floor(x_h) <= W // 2 - 2) & interior
    assert band.sum() >= 4 * H                                            # several columns wide
    rng = np.random.default_rng(3)
    m = rng.uniform(0.0, 2.0, (W, H, 3)).astype(np.float32)
    hist_c = np.concatenate([rng.uniform(0.0, 2.0, (W, H, 3)), np.full((W, H, 1), 5.0)], axis=-1).astype(np.float32)
    out, rp = hr.blend(m, 3, dist, cam, hist_c, hist_d, hcam, details=True)
    assert (rp["w"][band] == 0).all() and (out[band][:, :3].view(np.uint32) == m[band].view(np.uint32)).all() and (out[band][:, 3] == 3).all()
    assert (rp["w"][interior & ~band] > 0).all()
    assert (out[interior & ~band][:, 3] > 3).all()


def test_a_camera_turned_around_finds_no_history():
    p = params()
    cam = hr.camera(p, W, H)
    back = params(look=tuple(2 * np.array(p.camera_pos) - np.array(p.look_at)))
    hcam = hr.camera(back, W, H)
    dist = sphere_distance(cam)
    rng = np.random.default_rng(4)
    m = rng.uniform(0.0, 2.0, (W, H, 3)).astype(np.float32)
    hist_c = np.ones((W, H, 4), np.float32)
    out, rp = hr.blend(m, 2, dist, cam, hist_c, np.zeros((W, H), np.float32), hcam, details=True)
    assert (rp["z"] <= 0).all() and not rp["have"].any()
    assert (out[..., :3].view(np.uint32) == m.view(np.uint32)).all() and (out[..., 3] == 2).all()


def test_a_long_frame_outweighs_its_history():
    p = params()
    cam, hcam = hr.camera(yawed(p, 1.5), W, H), hr.camera(p, W, H)
    dist, hist_d = sphere_distance(cam), sphere_distance(hcam)
    rng = np.random.default_rng(5)
    m = rng.uniform(0.0, 2.0, (W, H, 3)).astype(np.float32)
    mh = 8.0
    hist_c = np.concatenate([rng.uniform(0.0, 2.0, (W, H, 3)), rng.uniform(0.5, 40.0, (W, H, 1))], axis=-1).astype(np.float32)
    n = int(64 * mh)
    out, rp = hr.blend(m, n, dist, cam, hist_c, hist_d, hcam, max_history=mh, details=True)
    assert rp["have"].mean() > 0.9 and (rp["w"] <= mh).all()
    h = rp["h"].astype(np.float64)
    m64 = m.astype(np.float64)
    # out - m = (h - m) w / (n + w) with w <= max_history; four f32 roundings of quantities no larger than max(|m|, |h|)
    bound = np.abs(h - m64) / 65.0 + 2.0 ** -22 * np.maximum(np.abs(h), np.abs(m64))
    have = rp["have"]
    assert (np.abs(out[..., :3].astype(np.float64) - m64)[have] <= bound[have]).all()


def test_a_zoom_keeps_the_optical_axis():
    p = params()
    wide = params(fov=p.fov * 1.3)
    cam, hcam = hr.camera(p, W, H), hr.camera(wide, W, H)
    axis = W / 2 - 0.5, H / 2 - 0.5
    _, xo, yo = hr.project([cam["d"][k] for k in range(3)], hcam, W, H)   # the optical axis itself
    assert abs(xo - axis[0]) < 1e-3 and abs(yo - axis[1]) < 1e-3
    dist = sphere_distance(cam)
    rp = hr.reproject(dist, cam, np.ones((W, H, 4), np.float32), sphere_distance(hcam), hcam)
    for u in (W // 2 - 1, W // 2):
        for v in (H // 2 - 1, H // 2):                                   # the four pixels about the axis keep their side of it, 1.3 times closer
            assert abs((rp["xo"][u, v] - axis[0]) - (u - axis[0]) / 1.3) < 1e-3
            assert abs((rp["yo"][u, v] - axis[1]) - (v - axis[1]) / 1.3) < 1e-3
    assert rp["have"][W // 2, H // 2]
