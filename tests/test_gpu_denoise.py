"""The denoiser of the display path (include/digital_earth_denoise.h): the GPU filter equals its float64 restatement; the guides are the
analytic ones on constant maps; the HDR sums and the display with the denoiser off do not change by a bit; the denoised display is the existing transform
of the filtered mean; the variance-source rule; quality against a high-spp reference of another seed; edges survive; every refusal answers its code."""
import ctypes
import os

import numpy as np
import pytest

import denoise_f64 as dn

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESETS = {"default": None, "florida": "config - florida.txt", "sunset": "config - sunset hurricane.txt", "apollo": "config - Apollo 11.txt"}
PLANET_R = 6371e3
CLOUDS_LOWER, CLOUDS_UPPER, CLOUDS_DENSITY, CLOUDS_EXTINCT = 6371e3 + 4000.0, 6371e3 + 10000.0, 0.029, 0.1


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


def _renderer(R, W, H, view="default", seed=11, source="synthetic", **kw):
    r = R.Renderer((W, H), (0, 1, 0), texture_source=source, texture_size=(2048, 1024), seed=seed, **kw)
    if PRESETS[view]:
        from digital_earth_amd.earth_viewer import load_config
        load_config(os.path.join(ROOT, "digital_earth_amd", "data", "configs", PRESETS[view])).apply(r)
    else:
        r.set_fov(0.42)
    r.copy_textures()
    return r


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / np.sqrt((b ** 2).sum()))


def _frame(r, spp, denoise=True):
    if denoise:
        r.set_denoise(True)
    r.reset_framebuffer()
    left = spp
    while left > 0:
        r.accumulate(min(left, 256))
        left -= min(left, 256)


# ---------------------------------------------------------------- the filter against its restatement
def _random_inputs(W, H, rng, structured):
    g = np.zeros((W, H, 9), np.float32)
    if structured:
        u = np.arange(W)[:, None] / W
        v = np.arange(H)[None, :] / H
        cov = ((u - 0.5) ** 2 + (v - 0.5) ** 2 < 0.12).astype(np.float32)
        cov[np.abs(((u - 0.5) ** 2 + (v - 0.5) ** 2) - 0.12) < 0.01] = 0.5
        g[..., 0] = cov
        g[..., 1] = np.where(cov > 0, 2.0e7 - 5.0e6 * cov + 1.0e5 * u, 0.0)
        n = np.stack(np.broadcast_arrays(u - 0.5, v - 0.5, np.full((W, H), 0.6)), -1)
        n = n / np.linalg.norm(n, axis=-1, keepdims=True)
        g[..., 2:5] = np.where(cov[..., None] > 0, n, 0.0)
        g[..., 5:8] = np.where((u * 8).astype(int)[..., None] % 2 == 0, 0.2, 0.6) * cov[..., None]
        g[..., 8] = np.where((u - 0.3) ** 2 + (v - 0.6) ** 2 < 0.02, 0.3, 1.0)
        base = 0.05 + 0.5 * cov[..., None] * g[..., 5:8]
        mean = base + 0.05 * rng.standard_normal((W, H, 3))
        var = np.full((W, H), 0.05 ** 2 / 3.0) * rng.uniform(0.5, 1.5, (W, H))
    else:
        g[..., 0] = rng.choice([0.0, 0.25, 0.5, 0.75, 1.0], (W, H), p=[0.2, 0.05, 0.05, 0.05, 0.65])
        g[..., 1] = np.where(g[..., 0] > 0, rng.uniform(1e6, 2e7, (W, H)), 0.0)
        n = rng.standard_normal((W, H, 3)) * 0.2 + np.array([0.0, 0.0, 1.0])
        g[..., 2:5] = np.where(g[..., :1] > 0, n / np.linalg.norm(n, axis=-1, keepdims=True), 0.0)
        g[..., 5:8] = rng.uniform(0, 0.6, (W, H, 3))
        g[..., 8] = rng.uniform(0.2, 1.0, (W, H))
        mean = rng.uniform(0.0, 1.0, (W, H, 3))
        var = rng.uniform(0.0, 0.05, (W, H))
    return mean.astype(np.float32), var.astype(np.float32), g


@pytest.mark.parametrize("structured", [False, True])
def test_filter_matches_the_f64_restatement(R, structured):
    W, H = 96, 48
    r = _renderer(R, W, H, source="constant")
    rng = np.random.default_rng(7 + structured)
    mean, var, g = _random_inputs(W, H, rng, structured)
    for levels, sigma in ((5, 4.0), (2, 1.0)):
        got = r.debug_denoise(mean, var, g, levels=levels, sigma_luminance=sigma)
        c, v = dn.denoise(mean.astype(np.float64), var.astype(np.float64), g.astype(np.float64), levels, sigma)
        l2 = _rel_l2(got[..., :3], c)
        px = np.abs(got[..., :3] - c).max(-1) / np.maximum(np.abs(c).max(-1), 1e-6)
        l2v = _rel_l2(got[..., 3], v)
        print("filter vs f64 (structured=%s, levels %d): colour rel L2 %.3e, max per-pixel rel %.3e, variance rel L2 %.3e" % (structured, levels, l2, px.max(), l2v))
        # measured on gfx950: colour rel L2 <= 1.9e-7, per-pixel <= 3.8e-6, variance rel L2 <= 1.3e-6
        assert l2 <= 1e-6 and px.max() <= 2e-5
        assert l2v <= 1e-5
    r.close()


# ---------------------------------------------------------------- guides on constant maps
def _camera_rays(r):
    p = r._params
    W, H = r.image_res
    cam = np.array(p.camera_pos, np.float64)
    d = np.array(p.look_at, np.float64) - cam
    d /= np.linalg.norm(d)
    du = np.cross(d, np.array(p.up, np.float64)); du /= np.linalg.norm(du)
    dv = np.cross(du, d); dv /= np.linalg.norm(dv)
    fov, asp, scale = float(p.fov), W / H, float(p.aspect_scale)
    rays = []
    for k in range(4):
        ou, ov = (0.75 if k & 1 else 0.25), (0.75 if k & 2 else 0.25)
        u = np.arange(W)[:, None] + ou
        v = np.arange(H)[None, :] + ov
        fu = (2 * fov * u / H - fov * asp - 1e-5) * scale
        fv = 2 * fov * v / H - fov - 1e-5 + 0 * u
        dirs = d + fu[..., None] * du + fv[..., None] * dv
        rays.append(dirs / np.linalg.norm(dirs, axis=-1, keepdims=True))
    return cam, rays


def _sphere(cam, dirs, radius):
    b = dirs @ cam
    disc = b * b - cam @ cam + radius * radius
    s = np.sqrt(np.maximum(disc, 0.0))
    return -b - s, -b + s, disc


def test_guides_are_analytic_on_constant_maps(R):
    W, H = 128, 64
    r = _renderer(R, W, H, view="sunset", source="constant")
    r.set_texture(3, np.full((4, 4, 1), 255, np.uint8))      # a cloud map of 1.0 everywhere: the whole shell is cloud
    r.set_texture(1, np.zeros((1024, 2048, 1), np.uint8))     # flat terrain at a real map width: land_normal's step is pi R / width (pathtracer.py:20)
    g = r.fetch_guides()
    cam, rays = _camera_rays(r)
    hits, dist, clear, trans, hitpos, cosines = [], [], [], [], [], []
    for dirs in rays:
        t0, t1, disc = _sphere(cam, dirs, PLANET_R)
        hit = (disc > 0) & (t0 > 0)
        hits.append(hit)
        dist.append(np.where(hit, t0, 0.0))
        closest = np.sqrt(np.maximum(cam @ cam - (dirs @ cam) ** 2, 0.0))
        clear.append(np.abs(closest - PLANET_R))
        hitpos.append(cam + dirs * np.where(hit, t0, 0.0)[..., None])
        cosines.append(np.where(hit, np.abs((dirs * hitpos[-1]).sum(-1)) / PLANET_R, 1.0))
        c0, c1, cd = _sphere(cam, dirs, CLOUDS_UPPER)
        a, b = np.maximum(c0, 0.0), np.where(hit, np.minimum(c1, t0), c1)
        tau = np.zeros(a.shape)
        ok = (cd > 0) & (b > a)
        dt = np.where(ok, (b - a) / 64.0, 0.0)
        for i in range(64):
            pt = cam + dirs * (a + (i + 0.5) * dt)[..., None]
            rr = np.linalg.norm(pt, axis=-1)
            tau += np.where(ok & (rr > CLOUDS_LOWER) & (rr < CLOUDS_UPPER), CLOUDS_DENSITY, 0.0)
        trans.append(np.exp(-CLOUDS_EXTINCT * tau * dt))
    hits = np.array(hits)
    cov = hits.mean(0)
    clear_min = np.min(clear, axis=0)
    safe = clear_min > 5e3      # rays that graze the sphere within 5 km are left out: the sphere trace's 250 steps may end before it decides
    assert safe.mean() > 0.9 and (cov[safe] > 0).any() and (cov[safe] == 0).any()
    limb = safe & (cov > 0) & (cov < 1)
    print("guides: %d pixels, %d safe, %d partial-coverage limb pixels" % (W * H, safe.sum(), limb.sum()))
    assert (g[..., 0][safe] == cov[safe]).all()
    full = safe & (cov == 1)
    want_d = np.array(dist).sum(0) / np.maximum(hits.sum(0), 1)
    # the sphere trace stops within 1e-4 t of the surface along the normal (pathtracer.py:43), i.e. 1e-4 t / cos(incidence) along the ray: the rays that
    # meet the surface at more than 78 degrees from the normal are left out of the 1e-3 bound
    steep = full & (np.min(cosines, axis=0) >= 0.2)
    err_d = np.abs(g[..., 1][steep] / want_d[steep] - 1.0)
    print("distance: %d pixels, max rel err %.3e" % (steep.sum(), err_d.max()))
    assert steep.sum() > 0.5 * full.sum() and err_d.max() <= 1e-3
    radial = np.array(hitpos).sum(0)
    radial /= np.linalg.norm(radial, axis=-1, keepdims=True)
    assert ((g[..., 2:5] * radial).sum(-1)[full] >= 0.9999).all()
    # get_land_material on a grey map (greenery 0, no ocean): land * 0.8 + land * (255, 128, 64) / 255 * 0.2
    t = 128.0 / 255.0
    want_a = t * 0.8 + t * np.array([255.0, 128.0, 64.0]) / 255.0 * 0.2
    assert np.abs(g[..., 5:8][full] - want_a).max() <= 1e-5
    assert np.abs(g[..., 5:8][safe & (cov == 0)]).max() == 0.0
    want_t = np.mean(trans, axis=0)
    err = np.abs(g[..., 8] - want_t)[safe]
    print("cloud transmittance: max abs err %.3e, range %.3f .. %.3f" % (err.max(), want_t.min(), want_t.max()))
    assert err.max() <= 2e-3 and want_t.min() < 0.9
    r.close()


# ---------------------------------------------------------------- nothing else changes
@pytest.mark.parametrize("variant", [4, 6, 2])
def test_hdr_bits_do_not_change(R, variant):
    hdrs = []
    for on in (False, True):
        r = _renderer(R, 64, 32)
        r.set_kernel_variant(variant)
        _frame(r, 3, denoise=on)
        r.accumulate(2)
        if on:
            r.fetch_image()
            assert r.fetch_denoised_hdr().shape == (64, 32, 3)
        hdrs.append(r.fetch_hdr())
        r.close()
    assert (_bits(hdrs[0]) == _bits(hdrs[1])).all()


def test_display_after_turning_off_is_unchanged(R):
    a = _renderer(R, 64, 32)
    _frame(a, 4, denoise=False)
    want = a.fetch_image()
    b = _renderer(R, 64, 32)
    _frame(b, 4, denoise=True)
    den = b.fetch_image()
    b.set_denoise(False)
    assert b.denoise() is None
    got = b.fetch_image()
    assert (_bits(got) == _bits(want)).all()
    assert not (_bits(den) == _bits(want)).all()
    a.close(); b.close()


# ---------------------------------------------------------------- the display is the existing transform
def test_display_is_the_existing_transform_of_the_filtered_mean(R):
    W, H = 64, 32
    r = _renderer(R, W, H, view="sunset")
    _frame(r, 8)
    img = r.fetch_image()
    assert (_bits(r.fetch_image()) == _bits(img)).all()      # repeated calls: the same bits
    mean = r.fetch_denoised_hdr()
    o = _renderer(R, W, H, view="sunset")
    o.upload_hdr(mean, spp=1)
    check_img = o.fetch_image()
    assert (_bits(check_img) == _bits(img)).all()
    # pipelined fetches equal the synchronous ones
    for lag in (1, 2, 3):
        sync, piped = [], []
        _frame(r, 1)
        for k in range(4):
            r.accumulate(1)
            sync.append(r.fetch_image())
        _frame(r, 1)
        for k in range(4):
            r.accumulate(1)
            im = r.fetch_image(lag=lag)
            if im is not None:
                piped.append(im)
        piped += r.fetch_pending(all_images=True)
        assert len(piped) == 4
        for a, b in zip(sync, piped):
            assert (_bits(a) == _bits(b)).all(), lag
    r.close(); o.close()


# ---------------------------------------------------------------- the variance-source rule
def test_enabled_mid_frame_equals_an_upload(R):
    W, H = 64, 32
    a = _renderer(R, W, H)
    a.reset_framebuffer()
    a.accumulate(8)
    a.set_denoise(True)          # after the first accumulate: S2 incomplete, the spatial variance
    a.accumulate(4)
    img_a = a.fetch_image()
    hdr = a.fetch_hdr()
    b = _renderer(R, W, H)
    b.set_denoise(True)
    b.reset_framebuffer()
    b.upload_hdr(hdr, spp=12)
    img_b = b.fetch_image()
    assert (_bits(img_a) == _bits(img_b)).all()
    # and the restatement of the spatial rule agrees with the filtered mean
    got = a.fetch_denoised_hdr()
    c, _ = dn.denoise_frame(hdr.astype(np.float64), None, 12, a.fetch_guides().astype(np.float64), s2_complete=False)
    assert _rel_l2(got, c) <= 1e-4
    a.close(); b.close()


def test_temporal_rule_matches_the_restatement(R):
    W, H = 64, 32
    r = _renderer(R, W, H, view="sunset")
    _frame(r, 16)
    got = r.fetch_denoised_hdr()
    hdr = r.fetch_hdr()
    s2 = r.adaptive_moments()
    c, _ = dn.denoise_frame(hdr.astype(np.float64), s2.astype(np.float64), 16, r.fetch_guides().astype(np.float64))
    print("temporal rule vs f64: rel L2 %.3e" % _rel_l2(got, c))
    assert _rel_l2(got, c) <= 1e-5      # measured 8.9e-7
    r.close()


def test_adaptive_frame_at_threshold_0_equals_the_uniform_frame(R):
    W, H = 64, 32
    a = _renderer(R, W, H)
    a.set_denoise(True)
    a.reset_framebuffer()
    a.render_adaptive(0.0, 16, min_spp=4, round_spp=4)
    b = _renderer(R, W, H)
    _frame(b, 16)
    assert (_bits(a.fetch_hdr()) == _bits(b.fetch_hdr())).all()
    assert (_bits(a.fetch_image()) == _bits(b.fetch_image())).all()
    a.close(); b.close()


# ---------------------------------------------------------------- quality
@pytest.fixture(scope="module")
def references(R):
    refs = {}
    for view in PRESETS:
        r = _renderer(R, 256, 128, view=view, seed=1000)
        _frame(r, 4096, denoise=False)
        refs[view] = r.fetch_image()
        r.close()
    return refs


@pytest.mark.parametrize("view", list(PRESETS))
def test_quality_against_a_reference(R, references, view):
    ref = references[view]
    r = _renderer(R, 256, 128, view=view, seed=3)
    out = {}
    for spp in (1, 4, 16, 256):
        _frame(r, spp, denoise=True)
        den = r.fetch_image()
        r.set_denoise(False)
        raw = r.fetch_image()
        out[spp] = (_rel_l2(raw, ref), _rel_l2(den, ref))
    print("quality %s: " % view + ", ".join("%d spp raw %.4f den %.4f (x%.2f)" % (s, a, b, a / b) for s, (a, b) in out.items()))
    assert out[1][1] < out[1][0]
    assert out[4][1] <= 0.5 * out[4][0] and out[16][1] <= 0.5 * out[16][0]
    assert out[256][1] <= out[256][0]
    r.close()


# ---------------------------------------------------------------- edges survive
def _edge_width(img, ref):
    """The 10-90 % transition width (pixels) of the averaged edge profile: for each row (or column) the reference's strongest step fixes the edge, both
    images' luminance profiles +-10 px around it are averaged over the rows (sign-aligned), the width is measured on each average."""
    def lum(x):
        return x @ np.array([0.2126, 0.7152, 0.0722])
    yr, yi = lum(ref.astype(np.float64)), lum(img.astype(np.float64))
    best = None
    for axis in (0, 1):
        a, b = (yr, yi) if axis == 0 else (yr.T, yi.T)
        grad = np.abs(np.diff(a, axis=0))
        strength = grad.max(0)
        lines = np.argsort(strength)[::-1][: max(4, a.shape[1] // 4)]
        prof_r, prof_i = [], []
        for j in lines:
            k = int(np.argmax(grad[:, j]))
            if k < 10 or k + 11 > a.shape[0]:
                continue
            s = 1.0 if a[k + 1, j] > a[k, j] else -1.0
            prof_r.append(s * a[k - 10:k + 11, j]); prof_i.append(s * b[k - 10:k + 11, j])
        if len(prof_r) < 4:
            continue
        pr, pi = np.mean(prof_r, 0), np.mean(prof_i, 0)
        if best is None or (pr.max() - pr.min()) > best[0]:
            best = (pr.max() - pr.min(), pr, pi)
    def width(p):
        lo, hi = p[:5].mean(), p[-5:].mean()
        f = (p - lo) / (hi - lo)
        i10 = np.argmax(f >= 0.1); i90 = np.argmax(f >= 0.9)
        def frac(i, level):
            return i - 1 + (level - f[i - 1]) / (f[i] - f[i - 1]) if i > 0 and f[i] != f[i - 1] else float(i)
        return frac(i90, 0.9) - frac(i10, 0.1)
    return width(best[1]), width(best[2])      # (reference, image)


def _edge_scene(R, kind, seed):
    r = _renderer(R, 256, 128, view="sunset" if kind == "limb" else "default", seed=seed, source="constant" if kind != "limb" else "synthetic")
    if kind == "albedo":
        a = np.full((64, 128, 3), 40, np.uint8); a[:, ::16] = 220
        for k in range(1, 8):
            a[:, k::16] = 220
        r.set_texture(0, a)
    elif kind == "cloud":
        r.set_texture(0, np.full((4, 4, 3), 10, np.uint8))
        r.set_texture(2, np.full((4, 4, 1), 255, np.uint8))      # ocean everywhere: dark
        c = np.zeros((256, 512, 1), np.uint8)
        yy, xx = np.mgrid[0:256, 0:512]
        for cx in range(0, 512, 64):
            c[((xx - cx) ** 2 + (yy - 128) ** 2) < 24 ** 2] = 255
        r.set_texture(3, c)
    return r


@pytest.mark.parametrize("kind", ["albedo", "cloud", "limb"])
def test_edges_survive(R, kind):
    ref_r = _edge_scene(R, kind, seed=1000)
    _frame(ref_r, 4096, denoise=False)
    ref = ref_r.fetch_image()
    ref_r.close()
    r = _edge_scene(R, kind, seed=5)
    _frame(r, 16, denoise=True)
    img = r.fetch_image()
    r.close()
    w_ref, w_img = _edge_width(img, ref)
    print("edge %s: reference width %.2f px, denoised 16 spp %.2f px" % (kind, w_ref, w_img))
    assert w_img <= w_ref + 1.0


# ---------------------------------------------------------------- refusals
def test_refusals(R):
    from digital_earth_amd import _native
    r = _renderer(R, 64, 32)
    L, h = r._lib, r._h
    d = _native.DeDenoise()
    d.struct_bytes = ctypes.sizeof(d) + 4; d.levels = 5; d.sigma_luminance = 4.0
    assert L.de_set_denoise(h, ctypes.byref(d)) == ERR_INVALID
    d.struct_bytes = ctypes.sizeof(d)
    for lv, s in ((0, 4.0), (11, 4.0), (5, 0.0), (5, -1.0), (5, float("nan")), (5, float("inf"))):
        d.levels, d.sigma_luminance = lv, s
        assert L.de_set_denoise(h, ctypes.byref(d)) == ERR_INVALID, (lv, s)
    out = np.empty((64, 32, 3), np.float32)
    assert L.de_fetch_denoised_hdr(h, out.ctypes.data) == ERR_STATE       # the denoiser is off
    r.set_denoise(True)
    assert r.denoise() == dict(levels=5, sigma_luminance=4.0)
    r.reset_framebuffer()
    r.accumulate(1)
    r.fetch_image()
    img = np.empty((64, 32, 3), np.float32)
    # a tile partition
    assert L.de_accumulate(h, 1, ctypes.c_uint64(0), 0, 2) == 0
    assert L.de_fetch_image(h, img.ctypes.data) == ERR_STATE
    assert L.de_fetch_denoised_hdr(h, out.ctypes.data) == ERR_STATE
    assert L.de_accumulate(h, 1, ctypes.c_uint64(0), 0, 1) == 0
    assert L.de_fetch_image(h, img.ctypes.data) == 0
    # a sample partition
    assert L.de_set_sample_partition(h, 0, 2) == 0
    assert L.de_fetch_image(h, img.ctypes.data) == ERR_STATE
    assert L.de_fetch_image_begin(h) == ERR_STATE
    assert L.de_set_sample_partition(h, 0, 1) == 0
    # a display source
    ptr, n = ctypes.c_void_p(), ctypes.c_uint64()
    assert L.de_hdr_device_ptr(h, ctypes.byref(ptr), ctypes.byref(n)) == 0
    assert L.de_set_display_source(h, ptr) == 0
    assert L.de_fetch_image(h, img.ctypes.data) == ERR_STATE
    view = ctypes.POINTER(ctypes.c_float)()
    assert L.de_fetch_image_view(h, ctypes.byref(view)) == ERR_STATE
    dev = ctypes.c_void_p()
    assert L.de_render_to_image(h, ctypes.byref(dev)) == ERR_STATE
    assert L.de_set_display_source(h, None) == 0
    assert L.de_fetch_image(h, img.ctypes.data) == 0
    assert L.de_get_denoise(h, None) == ERR_INVALID
    r.close()
