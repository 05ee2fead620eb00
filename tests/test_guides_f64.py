"""The float64 statement of the denoiser's guides (tests/guides_f64.py) against the oracle's probes (Oracle.probe: the restatement's own intersect_land,
land_normal, get_land_material and get_clouds_density in float32), on the maps and views of tests/guides_scenes.py.  No GPU.

Each function meets its probe; outside the ambiguity mask the float32 probe and the float64 statement stop the sphere trace at the same step and make
the same density decisions; guides composed in float32 from the probes (the kernel's composition: ray generation, sphere intersections and sample
points in float32 numpy, the four-ray sums in float32) give the measured basis of the GPU bounds; and the mask leaves enough of every kind of pixel."""

import numpy as np
import pytest

import guides_f64 as gf
import guides_scenes as gs
from oracle import oracle_binding as ob

F = np.float32
SLOTS = dict(albedo=0, height=1, ocean=2, clouds=3)
CLAMP_FLAG = 1 << 1


@pytest.fixture(scope="module")
def maps():
    return gs.make_maps()


@pytest.fixture(scope="module")
def oracle(maps, lut_arrays):
    o = ob.Oracle(16, 8)
    cie, s2s, o3, crf, _ = lut_arrays
    o.upload_luts(cie, s2s, o3, crf)
    for name, slot in SLOTS.items():
        o.upload_texture(slot, maps[name])
    for slot in (4, 5):
        o.upload_texture(slot, np.zeros((1, 1, 1), np.uint8))
    o.upload_texture(6, np.zeros((1, 1, 3), np.uint8))
    yield o
    o.close()


def _configure(o, cam, clamp):
    p = o.get_params()
    p.land_height_scale = cam["land_height_scale"]
    p.topo_res_override = int(cam.get("topo_res") or 0)
    p.flags = CLAMP_FLAG if clamp else 0
    o.set_params(p)


@pytest.fixture(scope="module")
def references(maps):
    """(view, size, clamp) -> (guides, mask, rays) of the float64 statement, computed once."""
    made = {}

    def get(view, size, clamp):
        if (view, size, clamp) not in made:
            made[(view, size, clamp)] = gf.guides(maps, gs.VIEWS[view], size[0], size[1], clamp)
        return made[(view, size, clamp)]
    return get


# ---------------------------------------------------------------- the functions
def _points(rng, n, r_lo, r_hi):
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    # a share of them around the seam (+x, small z of either sign) and the poles
    d[: n // 4] = np.stack([np.abs(d[: n // 4, 0]) + 1.0, d[: n // 4, 1], 0.01 * d[: n // 4, 2]], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return (d * rng.uniform(r_lo, r_hi, (n, 1))).astype(F)


def test_sphere_uv_map_meets_the_oracle():
    rng = np.random.default_rng(1)
    n = _points(rng, 20000, 1.0, 1.0)
    n = (n / np.linalg.norm(n.astype(np.float64), axis=-1, keepdims=True)).astype(F)
    got = ob.evaluate("sphere_UV_map", n, 2).astype(np.float64)
    u, v = gf.sphere_UV_map(n.astype(np.float64))
    du = np.abs(got[:, 0] - u)
    du = np.minimum(du, 1.0 - du)            # u = 0 and u = 1 are the same meridian
    print("sphere_UV_map: max |du| %.2e, |dv| %.2e" % (du.max(), np.abs(got[:, 1] - v).max()))
    # the arithmetic contract's atan2 / asin: 8e-7 and 2.5e-7 rad (tests/test_oracle_kat.py), over 2 pi and pi, plus float32 rounding of a value near 1
    assert du.max() <= 8e-7 / (2 * np.pi) + 1.2e-7 and np.abs(got[:, 1] - v).max() <= 2.5e-7 / np.pi + 1.2e-7


@pytest.mark.parametrize("clamp", [False, True])
def test_scene_functions_meet_the_probes(oracle, maps, clamp):
    cam = gs.VIEWS["far"]
    _configure(oracle, cam, clamp)
    scale = cam["land_height_scale"]
    rng = np.random.default_rng(2)
    pos = _points(rng, 20000, gs.PLANET_R - 2e3, gs.PLANET_R + 60e3)
    p64 = pos.astype(np.float64)
    # land_sdf: the texel filter in both address modes.  float32: |pos| to 0.5 m, the filtered byte to 1e-6 of 255 -> scale * 3e-7, uv to 3e-7 * the
    # map's steepest slope per unit u (the seam's cliff aside: a point within 2e-6 of u = 0 | 1 is left out)
    u, _ = gf.sphere_UV_map(p64 / np.linalg.norm(p64, axis=-1, keepdims=True))
    away = np.minimum(u, 1.0 - u) > 2e-6
    got = oracle.probe("land_sdf", pos)[:, 0].astype(np.float64)
    err = np.abs(got - gf.land_sdf(maps["height"], p64, scale, clamp))[away]
    print("land_sdf (clamp=%s): max abs err %.3f m" % (clamp, err.max()))
    assert err.max() <= 2.0
    # land_normal: differences of three such values over e = 39 km (a metre in 39 km: 1 - dot below 1e-9); what shows is the float32 unit vector's own
    # length, 1 +- 2.5 ulp after the reciprocal and the products
    got = oracle.probe("land_normal", pos).astype(np.float64)
    dot = (got * gf.land_normal(maps["height"], maps["height"].shape[1], p64, scale, clamp)).sum(-1)[away]
    print("land_normal: min dot %.9f" % dot.min())
    assert dot.min() >= 1.0 - 3e-7
    # get_land_material: float32 rounding (5e-6 albedo, 2e-6 ocean) plus the uv error (2.5e-7, measured above) times the map's slope, times 8 for the
    # grade's largest gain (its saturation of 6.5).  More than a texel from the seam the slope is the interior's steepest step, the same in both modes; only
    # the points within a texel of u = 0 | 1 or of a pole in wrap mode, where the filter blends across the map's edge, get the edge's step.
    def slope(m, seam):
        m = m.astype(np.float64)
        du_, dv_ = np.abs(np.diff(m, axis=1)).max(), np.abs(np.diff(m, axis=0)).max()
        if seam:      # wrap mode blends column 0 with the last column, and at the poles the top row with the bottom row
            du_, dv_ = max(du_, np.abs(m[:, 0] - m[:, -1]).max()), max(dv_, np.abs(m[0] - m[-1]).max())
        return (du_ * m.shape[1] + dv_ * m.shape[0]) / 255.0 * 2.5e-7
    got = oracle.probe("land_material", pos).astype(np.float64)
    alb, ocean = gf.get_land_material(maps["albedo"], maps["ocean"], p64, clamp)
    _, v = gf.sphere_UV_map(p64 / np.linalg.norm(p64, axis=-1, keepdims=True))
    inner = away & (np.minimum(u, 1.0 - u) > 1.0 / gs.W_MAP) & (np.minimum(v, 1.0 - v) > 1.0 / gs.H_MAP)
    band = away & ~inner
    assert inner.sum() > 10000 and band.sum() > 20
    for name, sel, seam in (("interior", inner, False), ("within a texel of the seam or a pole", band, not clamp)):
        ea, eo = np.abs(got[:, :3] - alb)[sel].max(), np.abs(got[:, 3] - ocean)[sel].max()
        ta, to = 5e-6 + 8.0 * slope(maps["albedo"], seam), 2e-6 + slope(maps["ocean"], seam)
        print("land_material (clamp=%s), %s: albedo max abs err %.2e (tolerance %.2e), ocean %.2e (%.2e)" % (clamp, name, ea, ta, eo, to))
        assert ea <= ta and eo <= to
    # get_clouds_density: the same decisions away from the margins, the same value
    pos = _points(rng, 40000, gf.CLOUDS_LOWER - 500.0, gf.CLOUDS_UPPER + 500.0)
    want, edge = gf.get_clouds_density(maps["clouds"], pos.astype(np.float64), clamp, margins=True)
    got = oracle.probe("clouds_density", pos)[:, 0].astype(np.float64)
    ok = ~edge
    assert ok.mean() > 0.95 and (want[ok] > 0).sum() > 1000 and (want[ok] == 0).sum() > 1000
    assert ((got > 0) == (want > 0))[ok].all()
    c8 = maps["clouds"].astype(np.float64)
    tol_c = 1e-7 + gf.CLOUDS_DENSITY * np.abs(np.diff(np.concatenate([c8, c8[:, :1]], 1) if not clamp else c8, axis=1)).max() / 255.0 * c8.shape[1] * 2.5e-7
    print("clouds_density: max abs err %.2e (tolerance %.2e)" % (np.abs(got - want)[ok].max(), tol_c))
    assert np.abs(got - want)[ok].max() <= tol_c


# ---------------------------------------------------------------- the composition in float32 from the probes
def _dot32(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _rsi32(pos, dirs, r):
    b = _dot32(dirs, pos[None, :])
    with np.errstate(invalid="ignore"):
        s = np.sqrt(b * b - _dot32(pos, pos) + F(r) * F(r))
    return -b + -s, -b + s            # NaN for a miss, as in the restatement


def probe_guides(o, cam, W, H, clamp):
    """The guides composed the way guide_kernel composes them, every step in float32: per-ray dicts and the (W, H, 9) guides.  This mirrors the kernel
    on purpose and serves ONE end: to measure how far float32 lies from the float64 statement (the basis of the GPU bounds).  Agreement of the kernel
    with this function would be no evidence about the kernel; the kernel is checked against guides_f64 alone."""
    _configure(o, cam, clamp)
    d, du, dv = (x.astype(F) for x in gf.camera_basis(cam))
    pos = np.array(cam["pos"], F)
    fov, asp, scale = F(cam["fov"]), F(W / H), F(cam["aspect_scale"])
    rays = []
    for ou, ov in gf.OFFSETS:
        u = (np.arange(W, dtype=F)[:, None] + F(ou)) + F(0) * np.arange(H, dtype=F)[None, :]
        v = (np.arange(H, dtype=F)[None, :] + F(ov)) + F(0) * u
        fu = (F(2) * fov * u / F(H) - fov * asp - F(1e-5)) * scale
        fv = F(2) * fov * v / F(H) - fov - F(1e-5)
        dirs = (d + fu[..., None] * du + fv[..., None] * dv).reshape(-1, 3)
        dirs = dirs * (F(1) / np.sqrt(_dot32(dirs, dirs)))[:, None]
        n = dirs.shape[0]
        il = o.probe("intersect_land", np.concatenate([np.broadcast_to(pos, (n, 3)), dirs], 1))
        t, steps = il[:, 0], il[:, 1].astype(np.int64)
        hit = t > 0
        hp = pos + dirs[hit] * t[hit, None]
        normal, albedo = np.zeros((n, 3), F), np.zeros((n, 3), F)
        normal[hit] = o.probe("land_normal", hp)
        albedo[hit] = o.probe("land_material", hp)[:, :3]
        c0, c1 = _rsi32(pos, dirs, gf.CLOUDS_UPPER)
        with np.errstate(invalid="ignore"):
            t0 = np.where(c0 > 0, c0, F(0)).astype(F)                      # fmaxf(NaN, 0) = 0
            t1 = np.where(hit & ~(c1 < t), t, c1).astype(F)                # fminf(t1, t_land): NaN gives t_land
            ok = t1 > t0
        dt = np.where(ok, (t1 - t0) / F(gf.CLOUD_STEPS), F(0)).astype(F)
        ts = np.where(ok, t0, F(0))[:, None] + (np.arange(gf.CLOUD_STEPS, dtype=F) + F(0.5))[None, :] * dt[:, None]
        pts = (pos + dirs[:, None, :] * ts[..., None]).astype(F)
        dens = np.zeros((n, gf.CLOUD_STEPS), F)
        dens[ok] = o.probe("clouds_density", pts[ok].reshape(-1, 3)).reshape(-1, gf.CLOUD_STEPS)
        total = np.zeros(n, F)
        for i in range(gf.CLOUD_STEPS):
            total = total + dens[:, i]
        tau = F(gf.CLOUDS_EXTINCT) * total * dt
        trans = np.exp(-tau.astype(np.float64)).astype(F)                  # a correctly rounded expf stands in for HIP's
        rays.append(dict(hit=hit, t=t, steps=steps, normal=normal, albedo=albedo, trans=trans, cloud_density=dens))
    hits = np.sum([r["hit"] for r in rays], 0).astype(F)
    g = np.zeros((W * H, 9), F)
    g[:, 0] = hits * F(0.25)
    dist = sum((np.where(r["hit"], r["t"], F(0)) for r in rays), np.zeros(W * H, F))
    g[:, 1] = np.where(hits > 0, dist / np.maximum(hits, F(1)), F(0))
    nsum = sum((r["normal"] for r in rays), np.zeros((W * H, 3), F))
    ln = np.sqrt(_dot32(nsum, nsum))
    g[:, 2:5] = np.where(ln[:, None] > 0, nsum * (F(1) / np.maximum(ln, F(1e-30)))[:, None], F(0))
    g[:, 5:8] = sum((r["albedo"] for r in rays), np.zeros((W * H, 3), F)) * F(0.25)
    g[:, 8] = sum((r["trans"] for r in rays), np.zeros(W * H, F)) * F(0.25)
    return g.reshape(W, H, 9), rays


@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("size", gs.SIZES)
@pytest.mark.parametrize("view", list(gs.VIEWS))
def test_probe_guides_meet_the_f64_guides(oracle, references, view, size, clamp):
    W, H = size
    want, mask, rays64 = references(view, size, clamp)
    got, rays32 = probe_guides(oracle, gs.VIEWS[view], W, H, clamp)
    # per ray, outside the mask: the same hit decision, the same stopping step, the same density decisions (every figure is printed before any assertion)
    bad_hit = bad_step = bad_density = 0
    for r32, r64 in zip(rays32, rays64):
        ok = ~r64["ambiguous"]
        seg = ok & (r64["cloud_dt"] > 0)          # a ray without a segment in the shell takes no samples
        bad_hit += int((r32["hit"] != r64["hit"])[ok].sum())
        bad_step += int((r32["steps"] != r64["steps"])[ok].sum())
        bad_density += int((~((r32["cloud_density"] > 0) == (r64["cloud_density"] > 0)).all(-1))[seg].sum())
    print("decisions outside the mask, %s %dx%d clamp=%s: %d hit, %d step, %d density mismatches" % (view, W, H, clamp, bad_hit, bad_step, bad_density))
    um = ~mask
    dev = gs.deviations(got, want)
    bad_cov = int(dev["coverage"][um].sum())
    line = {k: float(dev[k][um].max()) for k in gs.BASIS}
    print("probe guides vs f64, %s %dx%d clamp=%s: " % (view, W, H, clamp) + ", ".join("%s %.3e" % kv for kv in line.items()))
    # measured (largest over the 16 cases): see guides_scenes.BASIS, which must hold them
    assert bad_cov == 0
    assert bad_hit == 0 and bad_step == 0 and bad_density == 0
    for k, v in line.items():
        assert v <= gs.BASIS[k], (k, v)


@pytest.mark.parametrize("view", list(gs.VIEWS))
def test_the_mask_leaves_enough_to_check(references, view):
    """From the reference alone: per view at most 15 % of the image is masked."""
    for size in gs.SIZES:
        for clamp in (False, True):
            _, mask, _ = references(view, size, clamp)
            print("%s %dx%d clamp=%s: %.1f %% masked" % (view, size[0], size[1], clamp, 100.0 * mask.mean()))
            assert mask.mean() <= 0.15


def test_every_kind_of_pixel_is_checked(references):
    """At least 50 unmasked pixels each of full and zero coverage, and at least 50 of partial coverage in EACH far view (the two sizes together;
    measured per case: far 18 at 80x40 and 51 at 128x64, seam 16 and 50)."""
    full = zero = 0
    for view in gs.VIEWS:
        part = 0
        for size in gs.SIZES:
            g, mask, _ = references(view, size, False)
            cov = g[..., 0][~mask]
            full += int((cov == 1).sum()); zero += int((cov == 0).sum())
            p = int(((cov > 0) & (cov < 1)).sum())
            print("%s %dx%d: %d unmasked pixels of partial coverage" % (view, size[0], size[1], p))
            part += p
        if view in gs.FAR_VIEWS:
            assert part >= 50, (view, part)
    print("unmasked pixels: %d full, %d zero coverage" % (full, zero))
    assert full >= 50 and zero >= 50


def test_the_seam_view_straddles_the_seam(references):
    for size in gs.SIZES:
        _, _, rays = references("seam", size, False)
        u = np.concatenate([r["hit_u"][r["hit"]] for r in rays])
        assert (u < 0.05).any() and (u > 0.95).any()
