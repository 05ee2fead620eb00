"""The denoiser's guides on relief maps, their invalidation, and a mixed-count adaptive frame through the filter.

guide_kernel against the float64 statement tests/guides_f64.py on the maps and views of tests/guides_scenes.py, compared on the pixels outside the
statement's ambiguity mask.  Bounds: four times the CPU-measured basis (guides_scenes.BASIS, measured and asserted by tests/test_guides_f64.py), never
looser than the constant-map test's.  Discrimination: references that are wrong in one respect must miss the GPU guides by more than ten times the
bound on at least 5 % of the unmasked pixels, so a kernel wrong in that respect could not pass.  Invalidation: the guides follow every input they
depend on without a reset and ignore the display's fields.  Mixed counts: an adaptive frame whose tiles stopped at different counts, some below the
temporal rule's 4 samples, meets denoise_f64 with the per-pixel n."""
import numpy as np
import pytest

import denoise_f64 as dn
import guides_f64 as gf
import guides_scenes as gs

pytestmark = pytest.mark.gpu

SLOTS = dict(albedo=0, height=1, ocean=2, clouds=3)
CLAMP_FLAG = 1 << 1


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def maps():
    return gs.make_maps()


@pytest.fixture(scope="module")
def references(maps):
    """(view, size, clamp) -> (guides, mask, rays) of the float64 statement, computed once and left unchanged."""
    made = {}

    def get(view, size, clamp):
        if (view, size, clamp) not in made:
            made[(view, size, clamp)] = gf.guides(maps, gs.VIEWS[view], size[0], size[1], clamp)
        return made[(view, size, clamp)]
    return get


def _apply(r, cam, clamp):
    r.set_camera_pos(*cam["pos"])
    r.set_look_at(*cam["look_at"])
    r.set_fov(cam["fov"])
    r.set_aspect_scale(cam["aspect_scale"])
    r.land_height_scale = cam["land_height_scale"]
    r.set_topo_res_override(int(cam.get("topo_res") or 0))
    r.set_flag(CLAMP_FLAG, clamp)


def _renderer(R, size, cam, clamp, maps, seed=11):
    r = R.Renderer(size, (0, 1, 0), texture_source="constant", seed=seed)
    for name, slot in SLOTS.items():
        r.set_texture(slot, maps[name])
    _apply(r, cam, clamp)
    r.copy_textures()
    return r


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / np.sqrt((b ** 2).sum()))


# ---------------------------------------------------------------- guides against float64
@pytest.mark.parametrize("clamp", [False, True])
@pytest.mark.parametrize("size", gs.SIZES)
@pytest.mark.parametrize("view", list(gs.VIEWS))
def test_guides_meet_the_f64_statement(R, maps, references, view, size, clamp):
    """Measured on gfx950 (largest over the 16 cases): see the comment at the assertions."""
    want, mask, _ = references(view, size, clamp)
    r = _renderer(R, size, gs.VIEWS[view], clamp, maps)
    got = r.fetch_guides()
    r.close()
    um = ~mask
    dev = gs.deviations(got, want)
    bound = gs.bounds()
    line = {k: float(dev[k][um].max()) for k in bound}
    print("guides vs f64, %s %dx%d clamp=%s: %d of %d unmasked pixels differ in coverage, " % (view, size[0], size[1], clamp, int(dev["coverage"][um].sum()), int(um.sum()))
          + ", ".join("%s %.3e (bound %.1e)" % (k, v, bound[k]) for k, v in line.items()))
    assert np.isfinite(got).all()
    assert not dev["coverage"][um].any()
    # measured on gfx950, largest over the 16 cases: coverage equal everywhere; distance 2.952e-6 (far 80x40), normal 1.007e-7, albedo 5.253e-6 (seam 80x40),
    # transmittance 4.915e-5 (seam 128x64)
    for k, v in line.items():
        assert v <= bound[k], (k, v, bound[k])


# ---------------------------------------------------------------- discrimination
def _miss_fraction(got, wrong, mask):
    """The share of unmasked pixels on which the GPU guides miss a reference by more than ten times the bound, in any channel (or in coverage)."""
    dev = gs.deviations(got, wrong)
    far = dev["coverage"].copy()
    for k, b in gs.bounds().items():
        far |= dev[k] > 10.0 * b
    return float(far[~mask].mean())


@pytest.fixture(scope="module")
def gpu_guides(R, maps):
    made = {}

    def get(view, size, clamp):
        if (view, size, clamp) not in made:
            r = _renderer(R, size, gs.VIEWS[view], clamp, maps)
            made[(view, size, clamp)] = r.fetch_guides()
            r.close()
        return made[(view, size, clamp)]
    return get


STUCK_V = ((0.25, 0.25), (0.75, 0.25), (0.25, 0.25), (0.75, 0.25))      # the v offset never leaves 0.25
STUCK_U = ((0.25, 0.25), (0.25, 0.75), (0.25, 0.25), (0.25, 0.75))      # the u offset never leaves 0.25
HALF_V = ((0.25, 0.5), (0.75, 0.5), (0.25, 0.5), (0.75, 0.5))


@pytest.mark.parametrize("view", ["near", "seam_close"])
def test_wrong_references_miss(R, maps, references, gpu_guides, view):
    """A reference with flat terrain, a constant cloud map or a sub-pixel offset that is stuck misses the GPU guides far beyond the bounds.
    Exchanging the u and v offsets proper permutes the same four rays and changes nothing, and offsets that stay centred on the pixel, such as
    (0.25 | 0.75, 0.5), differ in second order only: measured 0.0 % (near) and 1.1 % (seam_close) of the pixels on the CPU reference, printed here
    against the GPU too.  A stuck offset moves the pixel's mean ray by a quarter pixel, which is what an offset mix-up does in first order."""
    size = (128, 64)
    cam = gs.VIEWS[view]
    _, mask, _ = references(view, size, False)
    got = gpu_guides(view, size, False)
    wrong = {
        "flat terrain": gf.guides(dict(maps, height=np.zeros_like(maps["height"])), cam, size[0], size[1], False)[0],
        "constant cloud map": gf.guides(dict(maps, clouds=np.full_like(maps["clouds"], 128)), cam, size[0], size[1], False)[0],
        "u offset stuck": gf.guides(maps, cam, size[0], size[1], False, offsets=STUCK_U)[0],
        "v offset stuck": gf.guides(maps, cam, size[0], size[1], False, offsets=STUCK_V)[0],
    }
    centred = _miss_fraction(got, gf.guides(maps, cam, size[0], size[1], False, offsets=HALF_V)[0], mask)
    swapped = _miss_fraction(got, gf.guides(maps, cam, size[0], size[1], False, offsets=tuple((b, a) for a, b in gf.OFFSETS))[0], mask)
    out = {k: _miss_fraction(got, w, mask) for k, w in wrong.items()}
    print("discrimination, %s: " % view + ", ".join("%s %.3f" % kv for kv in out.items()) + "; offsets (0.25|0.75, 0.5) %.3f; u and v offsets exchanged %.3f" % (centred, swapped))
    # measured on gfx950: near: flat 1.000, constant cloud 0.736, u stuck 0.894, v stuck 0.906, centred offsets 0.000; seam_close: 1.000, 0.426, 1.000, 0.878,
    # centred offsets 0.005; exchanged offsets 0.000 on both
    assert swapped == 0.0
    for k, v in out.items():
        assert v >= 0.05, (k, v)


@pytest.mark.parametrize("size", gs.SIZES)
def test_the_other_address_mode_misses_on_the_seam(R, maps, references, gpu_guides, size):
    """On the close seam view the reference of the other address mode misses the GPU guides on at least 5 % of the unmasked pixels, both ways.  On the
    far seam view, whose hits span u < 0.05 to u > 0.95, the column of texels that the modes filter differently is too narrow for that (the CPU
    reference gives 0.0 % at 128x64): there the share is printed, not asserted."""
    for clamp in (False, True):
        _, mask, _ = references("seam_close", size, clamp)
        other, _, _ = references("seam_close", size, not clamp)
        share = _miss_fraction(gpu_guides("seam_close", size, clamp), other, mask)
        print("address mode, seam_close %dx%d: GPU clamp=%s against the reference of clamp=%s misses on %.3f of the unmasked pixels" % (size[0], size[1], clamp, not clamp, share))
        assert share >= 0.05          # measured on gfx950: 0.117 and 0.116 at 80x40, 0.120 and 0.123 at 128x64; the far seam view: 0.0000
    _, mask, rays = references("seam", size, False)
    u = np.concatenate([r["hit_u"][r["hit"]] for r in rays])
    assert (u < 0.05).any() and (u > 0.95).any()
    other, _, _ = references("seam", size, True)
    print("address mode, seam %dx%d: share %.4f" % (size[0], size[1], _miss_fraction(gpu_guides("seam", size, False), other, mask)))


# ---------------------------------------------------------------- invalidation
def test_guides_follow_their_inputs_without_a_reset(R, maps):
    size, view = (80, 40), "seam_close"
    cam = dict(gs.VIEWS[view])
    state = dict(maps)
    r = _renderer(R, size, cam, False, state)
    r.set_denoise(True)
    prev = r.fetch_guides()
    clamp = False

    def fresh():
        f = _renderer(R, size, cam, clamp, state)
        g = f.fetch_guides()
        f.close()
        return g

    assert (_bits(prev) == _bits(fresh())).all()
    moved = [c + d for c, d in zip(cam["pos"], (3.0e4, -2.0e4, 5.0e4))]
    changes = [
        ("camera position", lambda: (cam.update(pos=moved), r.set_camera_pos(*moved))),
        ("look-at", lambda: (cam.update(look_at=[1.0e5, 2.0e5, -1.0e5]), r.set_look_at(1.0e5, 2.0e5, -1.0e5))),
        ("fov", lambda: (cam.update(fov=float(np.float32(0.33))), r.set_fov(cam["fov"]))),
        ("aspect scale", lambda: (cam.update(aspect_scale=1.25), r.set_aspect_scale(1.25))),
        ("land_height_scale", lambda: (cam.update(land_height_scale=12000.0), setattr(r, "land_height_scale", 12000.0))),
        ("topo_res_override", lambda: (cam.update(topo_res=2048), r.set_topo_res_override(2048))),
        ("clamp flag", lambda: r.set_flag(CLAMP_FLAG, True)),
        ("height map", lambda: (state.update(height=np.ascontiguousarray(maps["height"][::-1])), r.set_texture(1, state["height"]))),
        ("albedo map", lambda: (state.update(albedo=np.ascontiguousarray(maps["albedo"][..., ::-1])), r.set_texture(0, state["albedo"]))),
        ("ocean map", lambda: (state.update(ocean=255 - maps["ocean"]), r.set_texture(2, state["ocean"]))),
        ("cloud map", lambda: (state.update(clouds=255 - maps["clouds"]), r.set_texture(3, state["clouds"]))),
    ]
    for name, change in changes:
        change()
        if name == "clamp flag":
            clamp = True
        got = r.fetch_guides()
        want = fresh()
        same = (_bits(got) == _bits(want)).all()
        moved_on = not (_bits(got) == _bits(prev)).all()
        print("after a change of the %s: equal to a fresh renderer's %s, different from before %s" % (name, same, moved_on))
        assert same, name
        assert moved_on, name
        prev = got
    # the display's fields leave them alone
    r.set_exposure(1.0); r.set_gamma(2.2); r.set_crf(1); r.vignette_strength = 0.3; r.vignette_radius = 0.2; r.set_sun_angle(0.3); r.set_sun_path_rot(0.5)
    assert (_bits(r.fetch_guides()) == _bits(prev)).all()
    r.close()


# ---------------------------------------------------------------- a frame of mixed counts
# With the hero-wavelength estimator a pixel's standard error after 2 to 16 samples is several times its luminance: thresholds up to 2 leave every lit
# tile running to max_spp (measured: tiles of 2 and 16 only); at 8 the lit tiles stop at every count from 4 to 16 and the black sky at 2.
ADAPTIVE_THRESHOLD = 8.0


def test_mixed_count_frame_meets_the_f64_filter(R, maps):
    """Measured on gfx950: rel L2 8.142e-7 with the per-pixel n, 3.635e-1 with n = current_spp everywhere; the tile counts are at the assertions."""
    W, H = 128, 64
    cam = dict(pos=[-15000000.0, 0.0, 15000000.0], look_at=[0.0, 0.0, 0.0], fov=0.42, aspect_scale=1.0, land_height_scale=7800.0, topo_res=0)

    def make():
        r = _renderer(R, (W, H), cam, False, maps)
        r.set_denoise(True)
        return r
    r = make()
    r.reset_framebuffer()
    r.render_adaptive(ADAPTIVE_THRESHOLD, 16, min_spp=2, round_spp=2)
    tiles = r.tile_spp()
    values, counts = np.unique(tiles, return_counts=True)
    print("tile counts: " + ", ".join("%d x %d" % (c, v) for v, c in zip(values, counts)) + "; current_spp %d" % r.current_spp)
    assert len(values) >= 3 and (tiles < 4).any() and (tiles >= 4).any()
    img = r.fetch_image()
    got = r.fetch_denoised_hdr()
    hdr, s2, guides = r.fetch_hdr().astype(np.float64), r.adaptive_moments().astype(np.float64), r.fetch_guides().astype(np.float64)
    n = np.repeat(np.repeat(tiles, 8, axis=0), 8, axis=1)
    assert n.shape == (W, H)
    want, _ = dn.denoise_frame(hdr, s2, n, guides)
    uniform, _ = dn.denoise_frame(hdr, s2, r.current_spp, guides)
    err, miss = _rel_l2(got, want), _rel_l2(got, uniform)
    print("mixed-count frame vs f64 with the per-pixel n: rel L2 %.3e; with n = current_spp everywhere: %.3e" % (err, miss))
    # measured on gfx950: tiles 95 x 2, 1 x 4, 6 x 6, 3 x 8, 5 x 10, 2 x 12, 4 x 14, 12 x 16 samples; rel L2 8.142e-7 against the per-pixel-n reference
    # (bound 1e-4, the project's spatial-rule bound); 3.635e-1 against the reference with n = current_spp (floor 1e-3)
    assert err <= 1e-4
    assert miss > 1e-3
    o = _renderer(R, (W, H), cam, False, maps)      # the denoiser off: the unchanged display of the filtered mean
    o.upload_hdr(got, spp=1)
    assert (_bits(o.fetch_image()) == _bits(img)).all()
    r.close(); o.close()
