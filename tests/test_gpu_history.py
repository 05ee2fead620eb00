"""History reprojection (include/digital_earth_history.h) on the GPU: the blend kernel equals the numpy float32 restatement
(tests/history_ref.py) bit for bit on synthetic inputs and through the whole display path from every source; the display is the unchanged transform
over the blended mean; off is untouched; what drops, keeps and chains the history; what it buys after a camera move; every error answers its code;
the pipelined window loop.

Sizes as in tests/test_gpu_bloom.py: 16x8, 80x56 and 208x120 (several workgroups, partial edge tiles).  Where the restatement's value is a NaN the
device must hold a NaN there; everything else is compared as bits."""
import ctypes

import numpy as np
import pytest

import bloom_ref as bl
import exposure_f64 as ae
import history_cases as hc
import history_f64 as h64
import history_ref as hr

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
SIZES = [(16, 8), (80, 56), (208, 120)]
POS, LOOK = (-15000000.0, 0.0, 15000000.0), (0.0, 0.0, 0.0)
FOV = float(np.radians(27.0) * 0.5)
F = np.float32


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def contexts(R):
    """Renderers on 1x1 maps (a smooth sphere under the atmosphere), shared per (size, key)."""
    made = {}

    def get(W, H, key=0):
        if (W, H, key) not in made:
            made[(W, H, key)] = R.Renderer((W, H), (0, 1, 0), texture_source="constant", seed=7)
            made[(W, H, key)].copy_textures()
        return made[(W, H, key)]
    yield get
    for r in made.values():
        r.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    """Bit for bit, except that a NaN of the restatement asks for a NaN (of any payload)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), what
    diff = (_bits(got) != _bits(want)) & ~nan
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


# ---------------------------------------------------------------- cameras
def _params(r, pos=POS, look=LOOK, fov=FOV):
    p = type(r._params).from_buffer_copy(bytes(r._params))
    for k in range(3):
        p.camera_pos[k], p.look_at[k] = float(pos[k]), float(look[k])
    p.up[0], p.up[1], p.up[2] = 0.0, 1.0, 0.0
    p.fov, p.aspect_scale = float(fov), 1.0
    return p


def _yaw(pos, look, angle):
    o = np.array(look, np.float64) - np.array(pos, np.float64)
    c, s = np.cos(angle), np.sin(angle)
    return tuple(np.array(pos) + np.array([c * o[0] + s * o[2], o[1], -s * o[0] + c * o[2]]))


def _cameras(r, H):
    """name -> de_params of the CURRENT camera; the history's is always "identical"."""
    px = 2.0 * FOV / H
    side = np.array([1.0, 0.0, 1.0]) / np.sqrt(2.0) * 3e5
    return {
        "identical": _params(r),
        "yaw 1.5 px": _params(r, look=_yaw(POS, LOOK, 1.5 * px)),
        "yaw 20 px": _params(r, look=_yaw(POS, LOOK, 20.0 * px)),
        "sideways": _params(r, pos=tuple(np.array(POS) + side), look=tuple(np.array(LOOK) + side)),
        "towards": _params(r, pos=tuple(np.array(POS) * 0.9)),
        "zoomed": _params(r, fov=FOV / 1.3),
        "turned around": _params(r, look=tuple(2.0 * np.array(POS) - np.array(LOOK))),
    }


def _sphere(cam, W, H, radius=6371e3):
    d = np.stack([x.astype(np.float64) for x in hr.rays(cam, W, H)], axis=-1)
    o = np.array([np.float64(x) for x in cam["cam"]])
    b = d @ o
    disc = b * b - (o @ o - radius * radius)
    t = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0.0)), 0.0)
    return np.where(t > 0, t, 0.0).astype(np.float32)


def _move(r, p):
    ctypes.memmove(ctypes.byref(r._params), ctypes.byref(p), ctypes.sizeof(p))
    r._push_params()


# ---------------------------------------------------------------- 1. the kernel against the restatement
_INPUTS = {}


def _inputs(r, W, H):
    """The arrays of test 1, made once per size: m with negative channels, n in {0, 1, 7}, a history with weights 0 .. 100 and NaN / Inf pixels."""
    if (W, H) in _INPUTS:
        return _INPUTS[(W, H)]
    rng = np.random.default_rng(77 * W + H)
    m = (np.exp2(rng.uniform(-8.0, 3.0, (W, H, 1))) * rng.uniform(-0.6, 2.0, (W, H, 3))).astype(np.float32)
    n = rng.choice(np.array([0, 1, 7], np.int32), (W, H))
    hist = (np.exp2(rng.uniform(-8.0, 3.0, (W, H, 1))) * rng.uniform(-0.6, 2.0, (W, H, 4))).astype(np.float32)
    hist[..., 3] = rng.choice(np.array([0.0, 0.5, 3.0, 31.0, 32.0, 100.0], np.float32), (W, H))
    k = rng.permutation(W * H)[:max(W * H // 16, 6)]
    values = np.array([(np.nan, 1, 1), (np.inf, 1, 1), (1, -np.inf, 0), (1, 1, np.nan), (np.inf, np.inf, np.inf)], np.float32)
    hist.reshape(-1, 4)[k, :3] = values[np.arange(len(k)) % len(values)]
    hist.reshape(-1, 4)[k, 3] = 5.0
    hcam = hr.camera(_params(r), W, H)
    hsphere = _sphere(hcam, W, H)
    holes = rng.uniform(size=(W, H)) < 0.15
    # the history's distance: the sphere, with random holes (no land) and random scale errors about the tolerance
    hist_d = np.where(holes, F(0), hsphere * rng.choice(np.array([1.0, 1.0, 0.985, 1.015, 0.97, 1.03], np.float32), (W, H))).astype(np.float32)
    step = (np.where(np.arange(W)[:, None] < W // 2, F(1e7), F(2e7)) + np.zeros((1, H), np.float32)).astype(np.float32)
    _INPUTS[(W, H)] = dict(m=m, n=n, hist=hist, hist_d=hist_d, hsphere=hsphere, step=step, rng=rng)
    return _INPUTS[(W, H)]


def _edge(base, tol, rng):
    """base scaled to both edges of the depth tolerance: (1 +- tol) to within a few f32 ulp (steps of tol 2^-16, about 5 ulp) on either side."""
    sign = rng.choice(np.array([-1.0, 1.0]), base.shape)
    k = rng.integers(-3, 4, base.shape)
    return (base.astype(np.float64) * (1.0 + sign * tol * (1.0 + k * 2.0 ** -16))).astype(np.float32)


@pytest.mark.parametrize("size", SIZES)
def test_kernel_equals_the_restatement_bit_for_bit(contexts, size):
    W, H = size
    r = contexts(W, H)
    x = _inputs(r, W, H)
    hp = _params(r)
    hcam = hr.camera(hp, W, H)
    seen = {"history": 0, "none": 0, "first": 0}
    for name, p in _cameras(r, H).items():
        cam = hr.camera(p, W, H)
        sphere = _sphere(cam, W, H)
        cases = {"mixed": (np.where(x["rng"].uniform(size=(W, H)) < 0.15, F(0), sphere).astype(np.float32), x["hist_d"])}
        if name in ("identical", "yaw 1.5 px"):
            cases["edge"] = (sphere, _edge(x["hsphere"], 0.02, x["rng"]))
        if name in ("identical", "sideways"):
            cases["step"] = (x["step"], x["step"])
        for case, (dist, hist_d) in cases.items():
            for kw in (dict(), dict(max_history=4.0, depth_tolerance=0.5)):
                got = r.debug_history(x["m"], x["n"], dist, p, x["hist"], hist_d, hp, **kw)
                want, rp = hr.blend(x["m"], x["n"], dist, cam, x["hist"], hist_d, hcam, details=True, **kw)
                _same(got, want, (name, case, kw))
                seen["history"] += int((rp["have"] & (x["n"] > 0)).sum())
                seen["first"] += int((rp["have"] & (x["n"] == 0)).sum())
                seen["none"] += int((~rp["have"]).sum())
                if name == "turned around":
                    assert not rp["have"].any()
                if case == "edge" and name == "identical" and not kw:
                    land = (dist > 0) & rp["have"]
                    assert 0.1 < (rp["B"][land] > 0.99).mean() < 0.9      # both sides of the tolerance occur
    assert min(seen.values()) > 0
    # no history yet: the mean and the count, whatever the camera
    got = r.debug_history(x["m"], x["n"], x["step"], hp)
    _same(got, hr.blend(x["m"], x["n"], x["step"], hcam))
    _same(got[..., :3], x["m"])


# ---------------------------------------------------------------- 1b. low cameras: the restatement bit for bit, the float64 statement within its budgets
def _low(r, key):
    """The device on one case of tests/history_cases.py against both references.  Returns the number of conditioned pixels compared with float64."""
    x = hc.case(*key)
    f = x["f64"]
    p = _params(r, x["p"].camera_pos, x["p"].look_at, x["p"].fov)
    hp = _params(r, x["hp"].camera_pos, x["hp"].look_at, x["hp"].fov)
    got = r.debug_history(x["m"], x["n"], x["dist"], p, x["hist"], x["hist_d"], hp)
    _same(got, hr.blend(x["m"], x["n"], x["dist"], x["cam"], x["hist"], x["hist_d"], x["hcam"]), key)
    ill = f["ill"]
    cond = ~(ill["depth"] | ill["z"] | ill["s"] | ill["B"]) if key[4] == "identical" else ~ill["any"]      # tests/test_history_f64.py: a still camera is on the grid
    err = np.abs(got[..., :3].astype(np.float64) - f["out"])
    bound = hc.blend_bound(x)
    assert (err[cond] <= bound[cond]).all(), (key, float((err[cond] / np.maximum(bound[cond], 1e-300)).max()))
    weight = min(float(x["hist"][0, 0, 3]), hr.DEFAULTS["max_history"])
    wb = np.where(f["full"], 0.0, 4.0 * f["pos"] * weight) + hc.K_BLEND * h64.EPS * f["Wout"]
    assert (np.abs(got[..., 3].astype(np.float64) - f["Wout"])[cond] <= wb[cond]).all(), key
    return int((cond & f["have"]).sum())


@pytest.mark.parametrize("size", hc.SIZES)
def test_kernel_at_low_cameras_equals_the_restatement_and_float64(contexts, size):
    r = contexts(*size)
    compared = 0
    for altitude in ("2 m", "100 m", "10 km", "100 m, oblique"):
        for fov in hc.FOVS:
            for view in ("horizon", "down"):
                for history in ("identical", "step 1 %", "step 30 % zoom 1.2"):
                    compared += _low(r, (size, altitude, fov, view, history))
    assert compared > 24 * size[0] * size[1]


def test_kernel_at_the_lowest_camera_with_partial_edge_tiles(contexts):
    """2 m, fov 0.05, a still camera: where the former expression was worst (2 px)."""
    r = contexts(208, 120)
    assert _low(r, ((208, 120), "2 m", 0.05, "horizon", "identical")) > 208 * 120 // 2


# ---------------------------------------------------------------- 2. the whole pipeline
def _start(r, p=None, **kw):
    """A fresh frame at camera p with the feature on and no history."""
    _move(r, p if p is not None else _params(r))
    r.set_history(True, **kw)
    r.reset_framebuffer()


def _display_elsewhere(other, r, mean, **features):
    """The unchanged display of a mean on a second context with r's parameters."""
    _move(other, r._params)
    other.reset_framebuffer()
    other.upload_hdr(np.ascontiguousarray(mean[..., :3]), 1)
    return other.fetch_image()


def _per_pixel(counts):
    return np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1)


@pytest.mark.parametrize("size", SIZES)
def test_pipeline_equals_the_restatement(contexts, size):
    W, H = size
    r, other = contexts(W, H), contexts(W, H, 1)
    pa = _params(r)
    pb = _params(r, look=_yaw(POS, LOOK, 1.5 * 2.0 * FOV / H))
    _start(r, pa)
    r.accumulate(7)
    first_image = r.fetch_image()
    hist = r.fetch_history_hdr()
    da = r.fetch_guides()[..., 1]
    _same(hist, hr.blend(hr.mean_of(r.fetch_hdr(), 7), 7, da, None))      # no history yet: the mean and its count
    assert (_bits(first_image) == _bits(_display_elsewhere(other, r, hist))).all()
    _move(r, pb)
    r.reset_framebuffer()
    r.accumulate(1)
    image = r.fetch_image()
    got = r.fetch_history_hdr()
    hdr = r.fetch_hdr()
    db = r.fetch_guides()[..., 1]
    want, rp = hr.blend(hr.mean_of(hdr, 1), 1, db, hr.camera(pb, W, H), hist, da, hr.camera(pa, W, H), details=True)
    _same(got, want)
    assert rp["have"].mean() > 0.5 and (got[..., 3][rp["have"]] > 1).all()
    assert (_bits(image) == _bits(_display_elsewhere(other, r, got))).all()
    assert (_bits(r.fetch_hdr()) == _bits(hdr)).all()                      # the sums are never written
    r.set_history(False)
    assert (_bits(r.fetch_image()) == _bits(_display_elsewhere(other, r, hr.mean_of(hdr, 1)))).all()      # off: the plain display again


@pytest.mark.parametrize("moved", [False, True])
def test_pipeline_at_a_low_camera(contexts, moved):
    """100 m above the sphere, looking at the horizon: the restatement bit for bit and the float64 statement within its budgets; a still camera keeps
    its picture in place (what it shows again is what it showed, to within G N S: the position budget of each axis times the first picture's steepest
    neighbour difference along that axis, G = Gx + Gy, which is at most twice the largest neighbour difference)."""
    W, H = 80, 56
    r = contexts(W, H)
    a, b = hc.camera_pair("100 m", FOV, "horizon", "step 1 %" if moved else "identical", H)
    pa, pb = _params(r, a.camera_pos, a.look_at, a.fov), _params(r, b.camera_pos, b.look_at, b.fov)
    _start(r, pa)
    r.accumulate(7)
    r.fetch_image()
    hist = r.fetch_history_hdr()
    da = r.fetch_guides()[..., 1]
    _move(r, pb)
    r.reset_framebuffer()
    r.accumulate(1)
    got = r.fetch_history_hdr()
    m = hr.mean_of(r.fetch_hdr(), 1)
    db = r.fetch_guides()[..., 1]
    r.set_history(False)
    cam, hcam = hr.camera(pb, W, H), hr.camera(pa, W, H)
    _same(got, hr.blend(m, 1, db, cam, hist, da, hcam))
    assert 0.2 < (db > 0).mean() < 0.8                                       # land and sky
    f = h64.history(cam, db, hist, da, hcam, hr.DEFAULTS["max_history"], hr.DEFAULTS["depth_tolerance"], m, 1, hc.N_POS, hc.N_LEN, hc.N_S)
    ill = f["ill"]
    cond = ~ill["any"] if moved else ~(ill["depth"] | ill["z"] | ill["s"] | ill["B"])
    assert cond.mean() >= 0.99
    # the first picture's steepest step between neighbours, in float64: what a pixel of position error can cost
    c = hist[..., :3].astype(np.float64)
    finite = np.isfinite(c).all()
    assert finite
    # a position error of e px in each axis moves a bilinear sample by at most (Gx + Gy) e: the steepest step along x plus the steepest along y
    G = float(np.abs(np.diff(c, axis=0)).max() + np.abs(np.diff(c, axis=1)).max())
    bound = hc.blend_bound(dict(f64=f, m=m), gradient=G)
    err = np.abs(got[..., :3].astype(np.float64) - f["out"])
    assert (err[cond] <= bound[cond]).all(), float((err[cond] / np.maximum(bound[cond], 1e-300)).max())
    assert (cond & f["have"]).mean() > 0.5
    if not moved:
        inner = np.zeros((W, H), bool)
        inner[1:-1, 1:-1] = True
        keep = cond & inner & f["land"] & f["have"]
        assert keep.sum() >= 100
        out, wout = got[..., :3].astype(np.float64), got[..., 3].astype(np.float64)
        w = wout - 1.0
        with np.errstate(all="ignore"):
            h = (out * wout[..., None] - m.astype(np.float64)) / w[..., None]
        # out's own roundings (K_BLEND of them, tests/history_cases.py) come back multiplied by Wout / w
        rounding = hc.K_BLEND * h64.EPS * np.maximum(np.abs(m.astype(np.float64)), np.abs(c)) * (wout / w)[..., None]
        moved_by = np.abs(h - c)
        assert (moved_by[keep] <= (G * f["pos"] + rounding)[keep]).all(), float((moved_by[keep] / (G * f["pos"] + rounding)[keep]).max())


def _two_frames(r, W, H, first, second):
    """Frame one at camera A (rendered by first(r)), a yaw, frame two (second(r)).  Returns (history of frame one, its distance, cameras)."""
    pa = _params(r)
    pb = _params(r, look=_yaw(POS, LOOK, 1.5 * 2.0 * FOV / H))
    _start(r, pa)
    first(r)
    hist = r.fetch_history_hdr()
    da = r.fetch_guides()[..., 1]
    _move(r, pb)
    r.reset_framebuffer()
    second(r)
    return hist, da, hr.camera(pa, W, H), hr.camera(pb, W, H)


def test_pipeline_reads_an_adaptive_frame_with_its_tile_counts(contexts):
    W, H = 80, 56
    r, other = contexts(W, H), contexts(W, H, 1)
    hist, da, ca, cb = _two_frames(r, W, H, lambda q: q.render_adaptive(0.25, 32, min_spp=4, round_spp=4), lambda q: q.render_adaptive(0.25, 32, min_spp=4, round_spp=4))
    counts = _per_pixel(r.tile_spp())
    assert len(np.unique(counts)) >= 2
    image = r.fetch_image()
    got = r.fetch_history_hdr()
    want = hr.blend(hr.mean_of(r.fetch_hdr(), counts), counts, r.fetch_guides()[..., 1], cb, hist, da, ca)
    _same(got, want)
    assert (got[..., 3] >= counts).all() and (got[..., 3] > counts).mean() > 0.5
    r.set_history(False)
    r.reset_framebuffer()
    assert (_bits(image) == _bits(_display_elsewhere(other, r, got))).all()


def test_pipeline_reads_the_denoised_mean(contexts):
    W, H = 80, 56
    r, other = contexts(W, H), contexts(W, H, 1)
    r.set_denoise(True)
    hist, da, ca, cb = _two_frames(r, W, H, lambda q: q.accumulate(7), lambda q: q.accumulate(2))
    image = r.fetch_image()
    got = r.fetch_history_hdr()
    filtered = r.fetch_denoised_hdr()
    want = hr.blend(filtered, 2, r.fetch_guides()[..., 1], cb, hist, da, ca)
    _same(got, want)
    assert (_bits(got[..., :3]) != _bits(hr.blend(hr.mean_of(r.fetch_hdr(), 2), 2, r.fetch_guides()[..., 1], cb, hist, da, ca)[..., :3])).any()
    r.set_denoise(False)
    r.set_history(False)
    assert (_bits(image) == _bits(_display_elsewhere(other, r, got))).all()


def test_auto_exposure_meters_the_blended_mean(contexts):
    W, H = 80, 56
    r, other = contexts(W, H), contexts(W, H, 1)
    manual = float(r.exposure[None])
    hist, da, ca, cb = _two_frames(r, W, H, lambda q: q.accumulate(7), lambda q: q.accumulate(1))
    r.set_auto_exposure(True)
    image = r.fetch_image()
    m = r.metering()
    got = r.fetch_history_hdr()
    _same(got, hr.blend(hr.mean_of(r.fetch_hdr(), 1), 1, r.fetch_guides()[..., 1], cb, hist, da, ca))
    want_h = ae.meter(got[..., :3], 1)
    assert (m["histogram"] == want_h["histogram"]).all()
    assert (m["histogram"] != ae.meter(r.fetch_hdr(), 1)["histogram"]).any()      # the plain mean would meter something else
    want = ae.Meter().update(want_h["histogram"], manual_exposure=manual)
    assert m["valid"] == want["valid"] and ae.ulps_f32(m["ev"], want["ev"]) <= 2.0
    r.set_auto_exposure(False)
    r.set_history(False)
    _move(other, r._params)
    other.set_exposure(m["ev"])
    other.reset_framebuffer()
    other.upload_hdr(np.ascontiguousarray(got[..., :3]), 1)
    assert (_bits(other.fetch_image()) == _bits(image)).all()
    other.set_exposure(manual)


def test_bloom_reads_the_blended_mean(contexts):
    W, H = 80, 56
    r, other = contexts(W, H), contexts(W, H, 1)
    kw = dict(intensity=0.4)
    hist, da, ca, cb = _two_frames(r, W, H, lambda q: q.accumulate(7), lambda q: q.accumulate(1))
    r.set_bloom(True, **kw)
    image = r.fetch_image()
    got = r.fetch_history_hdr()
    _same(got, hr.blend(hr.mean_of(r.fetch_hdr(), 1), 1, r.fetch_guides()[..., 1], cb, hist, da, ca))
    bloomed = r.fetch_bloom_hdr()
    _same(bloomed, bl.bloom(got[..., :3], 1, **kw)[0])
    r.set_bloom(False)
    r.set_history(False)
    assert (_bits(image) == _bits(_display_elsewhere(other, r, bloomed))).all()


# ---------------------------------------------------------------- 3. off is untouched
def test_off_is_untouched(R):
    def rendered():
        q = R.Renderer((64, 32), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=11)
        q.copy_textures()
        return q
    plain = rendered()
    plain.accumulate(4)
    hdr0, image0 = plain.fetch_hdr(), plain.fetch_image()
    assert plain.history() is None
    toggled = rendered()
    toggled.set_history(True)
    toggled.set_history(False)
    toggled.accumulate(4)
    assert toggled.history() is None
    assert (_bits(toggled.fetch_image()) == _bits(image0)).all() and (_bits(toggled.fetch_hdr()) == _bits(hdr0)).all()
    on = rendered()
    on.set_history(True)
    assert on.history() == dict(max_history=32.0, depth_tolerance=float(np.float32(0.02)))
    on.accumulate(4)
    assert (_bits(on.fetch_image()) == _bits(image0)).all()              # on, no history yet: the same picture
    assert (_bits(on.fetch_hdr()) == _bits(hdr0)).all()
    # a move: the sums of the new frame are the sums without the feature, always
    for q in (plain, on):
        q.set_look_at(2e5, 0.0, 0.0)
        q.reset_framebuffer()
        q.accumulate(2)
    shown = on.fetch_image()
    assert (_bits(on.fetch_hdr()) == _bits(plain.fetch_hdr())).all()
    assert (_bits(shown) != _bits(plain.fetch_image())).any()              # and the history shows
    on.set_history(False)
    assert (_bits(on.fetch_image()) == _bits(plain.fetch_image())).all()
    for q in (plain, toggled, on):
        q.close()


# ---------------------------------------------------------------- 4. state
def test_what_drops_keeps_and_chains_the_history(contexts):
    W, H = 80, 56
    r = contexts(W, H)
    px = 2.0 * FOV / H
    pa, pb, pc = _params(r), _params(r, look=_yaw(POS, LOOK, 1.5 * px)), _params(r, look=_yaw(POS, LOOK, 3.0 * px))
    ca, cb, cc = (hr.camera(p, W, H) for p in (pa, pb, pc))
    _start(r, pa)
    r.accumulate(7)
    hist = r.fetch_history_hdr()
    da = r.fetch_guides()[..., 1]
    _move(r, pb)
    r.reset_framebuffer()
    # before any sample: the reprojected picture is on screen
    got0 = r.fetch_history_hdr()
    db = r.fetch_guides()[..., 1]
    want0, rp = hr.blend(hr.mean_of(np.zeros((W, H, 3), np.float32), 0), 0, db, cb, hist, da, ca, details=True)
    _same(got0, want0)
    assert rp["have"].mean() > 0.9 and np.isfinite(got0[rp["have"]]).all()
    # that display made a candidate: a reset now would chain it; instead the frame goes on and is displayed again
    r.accumulate(1)
    got1 = r.fetch_history_hdr()
    _same(got1, hr.blend(hr.mean_of(r.fetch_hdr(), 1), 1, db, cb, hist, da, ca))
    # exposure and camera response are display-only: the history stays
    manual = float(r.exposure[None])
    r.set_exposure(manual + 1.0)
    r.set_crf(1)
    _same(r.fetch_history_hdr(), got1)
    r.set_exposure(manual)
    r.set_crf(0)
    # a second move chains: the history of the history
    _move(r, pc)
    r.reset_framebuffer()
    r.reset_framebuffer()                                                  # a reset without a display keeps the history
    r.accumulate(1)
    got2 = r.fetch_history_hdr()
    dc = r.fetch_guides()[..., 1]
    want2 = hr.blend(hr.mean_of(r.fetch_hdr(), 1), 1, dc, cc, got1, db, cb)
    _same(got2, want2)
    assert (got2[..., 3] > 1).mean() > 0.9

    def dropped():
        r.reset_framebuffer()
        r.accumulate(2)
        out = r.fetch_history_hdr()
        return (out[..., 3] == 2).all() and (_bits(out[..., :3]) == _bits(hr.mean_of(r.fetch_hdr(), 2))).all()
    # each of these drops it: the next output has Wout == n everywhere
    sun = float(r.sun_angle[None])
    r.set_sun_angle(sun + 0.1)
    assert dropped()
    r.set_sun_angle(sun)
    r.reset_framebuffer(); r.accumulate(1); r.fetch_image()
    r.reset_framebuffer(); r.accumulate(1)
    assert (r.fetch_history_hdr()[..., 3] > 1).any()                       # a history again
    r.copy_texture(0)                                                      # a map upload
    assert dropped()
    r.reset_framebuffer(); r.accumulate(1); r.fetch_image()
    r.set_history(True)                                                    # every call drops it
    assert dropped()
    r.set_history(False)


# ---------------------------------------------------------------- 5. what it buys
def test_history_beats_one_sample_after_a_small_move(R):
    W, H = 80, 56

    def make():
        q = R.Renderer((W, H), (0, 1, 0), texture_source="constant", seed=3)
        q.copy_textures()
        return q
    r = make()
    pa, pb = _params(r), _params(r, look=_yaw(POS, LOOK, 1.5 * 2.0 * FOV / H))
    # the condition, from the restatement alone: the nudge keeps at least 90 % of the pixels' history
    ca, cb = hr.camera(pa, W, H), hr.camera(pb, W, H)
    rp = hr.reproject(_sphere(cb, W, H), cb, np.ones((W, H, 4), np.float32), _sphere(ca, W, H), ca)
    assert (rp["w"] > 0).mean() >= 0.9
    images = {}
    for name in ("with", "without"):
        _move(r, pa)
        r.set_history(name == "with")
        r.reset_framebuffer()
        r.accumulate(16)
        r.fetch_image()
        _move(r, pb)
        r.reset_framebuffer()
        r.accumulate(1)
        images[name] = r.fetch_image().astype(np.float64)
        if name == "with":
            assert (r.fetch_history_hdr()[..., 3] > 1).mean() >= 0.9
    r.set_history(False)
    r.reset_framebuffer()
    r.seed = 1234
    r.accumulate(512)
    ref = r.fetch_image().astype(np.float64)
    r.close()
    err = {k: float(np.sqrt(((v - ref) ** 2).sum() / (ref ** 2).sum())) for k, v in images.items()}
    print("relative L2 against 512 spp: with history %.5f, without %.5f, ratio %.3f" % (err["with"], err["without"], err["with"] / err["without"]))
    assert err["with"] < err["without"]


# ---------------------------------------------------------------- 6. errors
def test_every_error_answers_its_code(R, contexts):
    from digital_earth_amd import _native
    W, H = 16, 8
    r = contexts(W, H)
    L, h = r._lib, r._h
    r.set_history(False)

    def settings(**kw):
        s = _native.DeHistory()
        s.struct_bytes = ctypes.sizeof(s)
        s.max_history, s.depth_tolerance = 32.0, 0.02
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    out = np.empty((W, H, 4), np.float32)
    assert L.de_fetch_history_hdr(h, out.ctypes.data) == ERR_STATE          # off
    nan, inf = float("nan"), float("inf")
    for kw in (dict(struct_bytes=8), dict(struct_bytes=16), dict(max_history=0.0), dict(max_history=-1.0), dict(max_history=nan), dict(max_history=inf),
               dict(depth_tolerance=0.0), dict(depth_tolerance=-0.1), dict(depth_tolerance=1.5), dict(depth_tolerance=nan), dict(depth_tolerance=inf)):
        assert L.de_set_history(h, ctypes.byref(settings(**kw))) == ERR_INVALID, kw
        assert r.history() is None                                            # a refused call changes nothing
    assert L.de_set_history(None, ctypes.byref(settings())) == ERR_INVALID
    assert L.de_get_history(h, None) == ERR_INVALID and L.de_fetch_history_hdr(h, None) == ERR_INVALID
    for kw in (dict(), dict(max_history=0.5), dict(max_history=1e6), dict(depth_tolerance=1.0), dict(depth_tolerance=1e-6)):
        assert L.de_set_history(h, ctypes.byref(settings(**kw))) == 0, kw
    r.reset_framebuffer()
    r.accumulate(1)
    assert L.de_fetch_history_hdr(h, out.ctypes.data) == 0
    assert L.de_set_history(h, None) == 0
    assert L.de_fetch_history_hdr(h, out.ctypes.data) == ERR_STATE
    got = _native.DeHistory()
    assert L.de_get_history(h, ctypes.byref(got)) == 0 and got.max_history == 0.0 and got.struct_bytes == 12
    # before the maps and the LUTs are set
    bare = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    assert bare._lib.de_set_history(bare._h, ctypes.byref(settings())) == 0
    assert bare._lib.de_fetch_history_hdr(bare._h, out.ctypes.data) == ERR_STATE
    image = np.empty((W, H, 3), np.float32)
    assert bare._lib.de_fetch_image(bare._h, image.ctypes.data) == ERR_STATE
    bare.close()
    # the debug entry
    p = _params(r)
    m, n, d = np.zeros((W, H, 3), np.float32), np.zeros((W, H), np.int32), np.zeros((W, H), np.float32)
    args = (m.ctypes.data, n.ctypes.data, d.ctypes.data, ctypes.byref(p), None, None, None)
    assert L.de_debug_history(h, *args, 32.0, 0.02, out.ctypes.data) == 0
    assert L.de_debug_history(h, *args, 0.0, 0.02, out.ctypes.data) == ERR_INVALID
    assert L.de_debug_history(h, *args, 32.0, 1.5, out.ctypes.data) == ERR_INVALID
    assert L.de_debug_history(h, *args, 32.0, 0.02, None) == ERR_INVALID
    hc = np.zeros((W, H, 4), np.float32)
    assert L.de_debug_history(h, m.ctypes.data, n.ctypes.data, d.ctypes.data, ctypes.byref(p), hc.ctypes.data, None, None, 32.0, 0.02, out.ctypes.data) == ERR_INVALID


# ---------------------------------------------------------------- 7. the pipelined window loop
@pytest.mark.parametrize("lag", [1, 2, 3])
def test_pipelined_fetches_give_the_synchronous_bits(contexts, lag):
    W, H = 80, 56
    r = contexts(W, H)
    px = 2.0 * FOV / H
    moves = {2: _params(r, look=_yaw(POS, LOOK, 1.5 * px)), 4: _params(r, look=_yaw(POS, LOOK, 4.0 * px))}

    def loop(lagged):
        _start(r)
        seq = []
        for k in range(7):
            if k in moves:
                _move(r, moves[k])
                r.reset_framebuffer()
            r.accumulate(1)
            seq.append(r.fetch_image(lag=lagged))
        if lagged:
            assert all(x is None for x in seq[:lagged])
            seq = seq[lagged:] + r.fetch_pending(all_images=True)
        return [np.array(x) for x in seq]
    sync = loop(0)
    final = r.fetch_history_hdr()
    piped = loop(lag)
    assert len(piped) == len(sync) == 7
    for k in range(7):
        assert (_bits(piped[k]) == _bits(sync[k])).all(), k
    _same(r.fetch_history_hdr(), final)
    assert (_bits(sync[2]) != _bits(sync[1])).any()
    r.set_history(False)


def test_earth_viewer_passes_the_option_through():
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(64, 32), texture_source="constant", seed=5)
    v = EarthViewer(history=dict(max_history=8.0), **kw)
    assert v.renderer.history() == dict(max_history=8.0, depth_tolerance=float(np.float32(0.02)))
    plain = EarthViewer(**kw)
    assert plain.renderer.history() is None
    a = [v.frame(spp=1).copy(), None, None]
    b = [plain.frame(spp=1).copy(), None, None]
    for q in (v, plain):
        q.camera.rotate(0.002, 0.0)
    for k in (1, 2):                          # frame 1 pushes the camera and resets after its display; frame 2 is the first of the new view
        a[k], b[k] = v.frame(spp=1).copy(), plain.frame(spp=1).copy()
    assert (_bits(a[0]) == _bits(b[0])).all() and (_bits(a[2]) != _bits(b[2])).any()
    v.close(); plain.close()
