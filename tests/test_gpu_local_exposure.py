"""Local exposure (include/digital_earth_local_exposure.h) on the GPU: the dodged mean equals the numpy float32 restatement
(tests/local_exposure_ref.py, with the device's own de_log and de_pow injected through Renderer.debug_math) bit for bit, on the test hook and from
every source the display reads; the display is the unchanged transform over it; the anchor follows the metered exposure; the stage reads the bloom's
composite; off, never on and both strengths 0 leave every bit alone; the 8-bit output and the pipelined window loop inherit it.

Sizes: 16x8 admits two levels; 64x32 is the plain case; 80x56 has the levels 40x28, 20x14, 10x7, 5x4 and 3x2 (odd widths and heights); 208x120 has
several workgroups per level and partial edge tiles (104x60, 52x30, 26x15, 13x8, 7x4, 4x2).

Where the restatement's value is a NaN (only at a pixel whose own input holds one) the device must hold a NaN there; everything else is compared as bits."""
import numpy as np
import pytest

import local_exposure_ref as lx

pytestmark = pytest.mark.gpu

SIZES = [(16, 8), (64, 32), (80, 56), (208, 120)]
SETTINGS = {
    "defaults": dict(),
    "one level": dict(levels=1),
    "not edge-aware": dict(sigma=1e9),
    "clamp bites": dict(max_ev=0.5),
    "no shadows": dict(shadows=0.0),
}
EXPOSURE_SCALE = float(np.float32(2.88))      # the anchor 0.18 / 2.88 = 2^-4 lies between the two sides of the step and in the middle of the random range
TAUS = (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01)

_INPUTS = {}


def inputs(W, H):
    """name -> (W, H, 3) float32 means, made once per size (tools/local_exposure_host_check.py runs the same ones on the host)."""
    if (W, H) in _INPUTS:
        return _INPUTS[(W, H)]
    rng = np.random.default_rng(7000 * W + H)
    # uniform in log luminance over 12 stops, 2^-10 .. 2^2, with some chroma
    random = (np.exp2(rng.uniform(-10.0, 2.0, (W, H, 1))) * rng.uniform(0.6, 1.4, (W, H, 3))).astype(np.float32)
    # a vertical edge of 4 stops, a little texture on both sides
    step = np.where(np.arange(W)[:, None, None] < W // 2, np.float32(0.02), np.float32(0.32)) * rng.uniform(0.9, 1.1, (W, H, 3)).astype(np.float32)
    constant = np.full((W, H, 3), 0.4, np.float32)
    # a block of black space and single pixels that are not light, at the corners and along the right edge's last group of four too
    dirty = random.copy()
    dirty[W // 4:W // 4 + max(W // 3, 3), H // 4:H // 4 + max(H // 3, 3)] = 0.0
    bad = np.array([(np.nan, 1, 1), (np.inf, 1, 1), (-1.0, -2.0, -0.5), (1, np.nan, np.nan), (np.inf, np.inf, np.inf), (0, 0, 0), (1e-9, 1e-9, 1e-9), (-np.inf, 0, 0)], np.float32)
    spots = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W - 1, H // 2), (W - 2, H // 2 + 1), (W - 3, 1), (W - 4, H - 2), (W // 2, H // 2), (W // 2 + 1, H // 2),
             (1, H // 2), (W // 3, 0)]
    for k, (i, j) in enumerate(spots):
        dirty[i, j] = bad[k % len(bad)]
    _INPUTS[(W, H)] = dict(random=random, step=step.astype(np.float32), constant=constant, dirty=dirty)
    return _INPUTS[(W, H)]


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def contexts(R):
    """One Renderer on 1x1 maps per size, shared by the tests that only upload sums and display."""
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[(W, H)] = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
            made[(W, H)].copy_textures()
        return made[(W, H)]
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


def device_math(r):
    """The device's own de_log and de_pow(2, .) as the restatement's two parameters."""
    return dict(log=lambda x: r.debug_math(1, x), pow2=lambda e: r.debug_math(6, np.full(np.shape(e), 2.0, np.float32), e))


def scale_of(r, ev):
    """exposure_scale as setup_kernel and the meter make it: de_pow(2, ev)."""
    return float(r.debug_math(6, np.array([2.0], np.float32), np.array([ev], np.float32))[0])


# ---------------------------------------------------------------- 1. the hook, bit for bit
@pytest.mark.parametrize("size", SIZES)
def test_hook_equals_the_restatement_bit_for_bit(contexts, size):
    W, H = size
    r = contexts(W, H)
    dm = device_math(r)
    for name, mean in inputs(W, H).items():
        for setting, kw in SETTINGS.items():
            got = r.debug_local_exposure(mean, EXPOSURE_SCALE, **kw)
            want, g = lx.local_exposure(mean, 1, EXPOSURE_SCALE, **kw, **dm)
            _same(got, want, (name, setting))
            if name == "constant":
                assert (got == got[0, 0, 0]).all()                           # every pixel of every level sees the same values, clamped edges included
            if name == "random" and setting == "defaults":
                assert (g != 1).any()
            if name == "step" and setting == "defaults":
                assert (g > 1).any() and (g < 1).any()                       # both strengths acted: the dark side is dodged, the bright side burned
            if name == "step" and setting == "clamp bites":
                assert (g == r.debug_math(6, np.full(1, 2.0, np.float32), np.array([-0.5], np.float32))[0]).mean() > 0.4      # the bright side sits on the bound
    assert r.local_exposure is None                                          # the hook does not turn the feature on


def test_levels_are_capped_by_the_image(contexts):
    """16x8 admits two levels: asking for 2, 6 or 10 gives the same bits, and 1 gives others."""
    r = contexts(16, 8)
    mean = inputs(16, 8)["random"]
    got = {levels: r.debug_local_exposure(mean, EXPOSURE_SCALE, levels=levels) for levels in (1, 2, 6, 10)}
    assert (_bits(got[2]) == _bits(got[6])).all() and (_bits(got[2]) == _bits(got[10])).all()
    assert (_bits(got[1]) != _bits(got[2])).any()


def test_unaligned_display_source_takes_the_scalar_loads(R):
    """A second context's buffer as the display source, offset by one float (4 bytes): no longer 16-byte aligned."""
    W, H = 64, 32
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    other = R.Renderer((W, H + 8), (0, 1, 0), texture_source="constant")      # larger: the shifted window stays inside it
    r.copy_textures()
    rng = np.random.default_rng(5)
    big = (np.exp2(rng.uniform(-10.0, 2.0, (W, H + 8, 1))) * rng.uniform(0.6, 1.4, (W, H + 8, 3))).astype(np.float32)
    other.upload_hdr(big, 1)
    own = np.full((W, H, 3), 0.4, np.float32)
    r.upload_hdr(own, 5)
    ptr, _ = other.hdr_device_pointer()
    scale = scale_of(r, float(r.exposure[None]))
    r.set_local_exposure(True)
    for offset_floats in (1, 0):
        r.set_display_source(ptr + 4 * offset_floats)
        on = r.fetch_image()
        got = r.fetch_local_exposure_hdr()
        flat = np.ascontiguousarray(big.transpose(1, 0, 2)).ravel()              # the device layout [H][W][3]
        seen = flat[offset_floats:offset_floats + W * H * 3].reshape(H, W, 3).transpose(1, 0, 2)
        assert (_bits(r.fetch_hdr()) == _bits(seen)).all()
        _same(got, lx.local_exposure(seen, 5, scale, **device_math(r))[0], offset_floats)
        r.set_display_source(None)
        r.set_local_exposure(False)
        r.upload_hdr(got, 1)
        assert (_bits(r.fetch_image()) == _bits(on)).all()
        r.upload_hdr(own, 5)
        r.set_local_exposure(True)
    r.close(); other.close()


@pytest.fixture(scope="module")
def wide(R):
    """144x72 reading a second context's buffer: the levels are 72x36, 36x18, 18x9, 9x5, 5x3 and 3x2 — level 1 spans several 16-output tiles in both
    axes and is wider than the 34-column staged tile, the widths and heights turn odd, and the plan stops at six levels whatever is asked for."""
    W, H = 144, 72
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    other = R.Renderer((W, H + 8), (0, 1, 0), texture_source="constant")      # larger: the shifted window stays inside it
    r.copy_textures()
    rng = np.random.default_rng(144)
    big = (np.exp2(rng.uniform(-10.0, 2.0, (W, H + 8, 1))) * rng.uniform(0.6, 1.4, (W, H + 8, 3))).astype(np.float32)
    other.upload_hdr(big, 1)
    r.upload_hdr(np.full((W, H, 3), 0.4, np.float32), 3)
    yield r, other, np.ascontiguousarray(big.transpose(1, 0, 2)).ravel()      # the device layout [H][W][3]
    r.close(); other.close()


@pytest.mark.parametrize("offset_floats", [0, 1])
@pytest.mark.parametrize("levels", [1, 2, 10])
def test_pyramid_at_144x72(wide, levels, offset_floats):
    """The source aligned, and offset by one float (no longer 16-byte aligned: the scalar loads)."""
    W, H = 144, 72
    r, other, flat = wide
    ptr, _ = other.hdr_device_pointer()
    assert lx.levels_used(W, H, levels) == min(levels, 6)
    r.set_display_source(ptr + 4 * offset_floats)
    r.set_local_exposure(True, levels=levels)
    got = r.fetch_local_exposure_hdr()
    seen = flat[offset_floats:offset_floats + W * H * 3].reshape(H, W, 3).transpose(1, 0, 2)
    r.set_local_exposure(False)
    r.set_display_source(None)
    _same(got, lx.local_exposure(seen, 3, scale_of(r, float(r.exposure[None])), levels=levels, **device_math(r))[0])


# ---------------------------------------------------------------- 2. a rendered frame
def _rendered(R, seed=11, spp=2):
    r = R.Renderer((64, 32), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=seed)
    r.set_fov(0.42)
    r.copy_textures()
    r.accumulate(spp)
    return r


def _display_elsewhere(R, mean, like):
    """fetch_image of a second context after upload_hdr(mean, 1), with the stage off and `like`'s exposure."""
    o = R.Renderer((64, 32), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=11)
    o.copy_textures()
    o.set_exposure(float(like.exposure[None]))
    o.upload_hdr(mean, 1)
    image = o.fetch_image()
    o.close()
    return image


def test_frame_is_dodged_and_displayed_unchanged(R):
    r = _rendered(R)
    sums = r.fetch_hdr()
    r.set_local_exposure(True)
    image = r.fetch_image()
    got = r.fetch_local_exposure_hdr()
    want, g = lx.local_exposure(sums, 2, scale_of(r, float(r.exposure[None])), **device_math(r))
    _same(got, want)
    assert (g != 1).any()
    assert (_bits(image) == _bits(_display_elsewhere(R, got, r))).all()
    assert r.local_exposure == dict(highlights=0.5, shadows=0.25, sigma=1.0, max_ev=2.0, key=float(np.float32(0.18)), levels=6)
    r.close()


def test_anchor_follows_the_metered_exposure(R):
    r = _rendered(R)
    sums = r.fetch_hdr()
    manual = float(r.exposure[None])
    r.set_auto_exposure(True)
    r.set_local_exposure(True)
    image = r.fetch_image()
    ev = r.metering()["ev"]
    assert ev != manual
    got = r.fetch_local_exposure_hdr()
    assert r.metering()["ev"] == ev                                           # adapt = 1: metering again changes nothing
    _same(got, lx.local_exposure(sums, 2, scale_of(r, ev), **device_math(r))[0])
    assert (_bits(got) != _bits(lx.local_exposure(sums, 2, scale_of(r, manual), **device_math(r))[0])).any()
    r.set_exposure(ev)
    assert (_bits(image) == _bits(_display_elsewhere(R, got, r))).all()
    r.close()


def test_stage_reads_the_bloom(R):
    r = _rendered(R)
    r.set_bloom(True, intensity=0.4)
    r.set_local_exposure(True)
    image = r.fetch_image()
    bloomed = r.fetch_bloom_hdr()
    got = r.fetch_local_exposure_hdr()
    scale = scale_of(r, float(r.exposure[None]))
    _same(got, lx.local_exposure(bloomed, 1, scale, **device_math(r))[0])
    assert (_bits(got) != _bits(lx.local_exposure(r.fetch_hdr(), 2, scale, **device_math(r))[0])).any()
    assert (_bits(image) == _bits(_display_elsewhere(R, got, r))).all()
    r.close()


def test_stage_reads_an_adaptive_frame_with_its_tile_counts(R):
    r = R.Renderer((64, 32), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=11)
    r.set_fov(0.42)
    r.copy_textures()
    for tau in TAUS:
        r.reset_framebuffer()
        r.render_adaptive(tau, 32, min_spp=4, round_spp=4)
        counts = r.tile_spp()
        if len(np.unique(counts)) >= 2:
            break
    else:
        pytest.fail("no threshold of %s spreads the tile counts" % (TAUS,))
    r.set_local_exposure(True)
    image = r.fetch_image()
    got = r.fetch_local_exposure_hdr()
    per_pixel = np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1)
    hdr = r.fetch_hdr()
    scale = scale_of(r, float(r.exposure[None]))
    _same(got, lx.local_exposure(hdr, per_pixel, scale, **device_math(r))[0])
    assert (_bits(got) != _bits(lx.local_exposure(hdr, int(counts.max()), scale, **device_math(r))[0])).any()      # the frame's largest count would give something else
    assert (_bits(image) == _bits(_display_elsewhere(R, got, r))).all()
    r.close()


# ---------------------------------------------------------------- 3. no side effects
def test_off_never_on_and_zero_strengths_keep_every_bit(R):
    r = _rendered(R, spp=4)
    hdr0 = r.fetch_hdr()
    before = r.fetch_image()
    assert r.local_exposure is None
    r.set_local_exposure(True, highlights=0.0, shadows=0.0)
    assert (_bits(r.fetch_image()) == _bits(before)).all()                    # both strengths 0: a gain of exactly 1
    r.set_local_exposure(True)
    for _ in range(3):
        on = r.fetch_image()
        assert (_bits(r.fetch_hdr()) == _bits(hdr0)).all()                    # the sums are never written
    assert (_bits(on) != _bits(before)).any()
    r.set_local_exposure(False)
    assert r.local_exposure is None
    assert (_bits(r.fetch_image()) == _bits(before)).all()
    assert (_bits(r.fetch_hdr()) == _bits(hdr0)).all()
    with pytest.raises(R.DigitalEarthError) as e:
        r.fetch_local_exposure_hdr()
    assert e.value.code == -4
    fresh = _rendered(R, spp=4)                                               # a context that never heard of the feature
    assert (_bits(fresh.fetch_image()) == _bits(before)).all()
    fresh.close(); r.close()


def test_settings_out_of_range_are_refused(contexts):
    r = contexts(16, 8)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(highlights=-0.1), dict(highlights=1.5), dict(highlights=nan), dict(shadows=-0.1), dict(shadows=1.5), dict(shadows=nan), dict(sigma=0.0),
               dict(sigma=-1.0), dict(sigma=nan), dict(sigma=inf), dict(max_ev=-0.5), dict(max_ev=nan), dict(max_ev=inf), dict(key=0.0), dict(key=-1.0), dict(key=nan),
               dict(levels=0), dict(levels=11)):
        with pytest.raises(Exception) as e:
            r.set_local_exposure(True, **kw)
        assert getattr(e.value, "code", None) == -1, kw
        assert r.local_exposure is None                                       # a refused call changes nothing
    for kw in (dict(), dict(highlights=0.0), dict(highlights=1.0, shadows=1.0), dict(max_ev=0.0), dict(levels=1), dict(levels=10), dict(sigma=1e9)):
        r.set_local_exposure(True, **kw)
    r.set_local_exposure(False)


# ---------------------------------------------------------------- 4. what sits behind the display inherits it
def test_pixels_are_the_pixels_of_the_dodged_image(R):
    r = _rendered(R)
    r.set_local_exposure(True)
    image = r.fetch_image()
    assert (r.fetch_pixels() == r.debug_pixels(image)).all()
    r.set_local_exposure(False)
    assert (r.fetch_pixels() != r.debug_pixels(image)).any()
    r.close()


def test_earth_viewer_frame_loop_pipelined_with_local_exposure():
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(64, 32), texture_source="synthetic", texture_size=(1024, 512), seed=5)

    def script(k):
        return dict(sun_angle=0.9) if k == 2 else {}
    a = EarthViewer(local_exposure=True, **kw)
    assert a.renderer.local_exposure is not None
    sync = [a.frame(spp=1, **script(k)).copy() for k in range(4)]
    b = EarthViewer(local_exposure=dict(highlights=0.5), **kw)
    got = [b.frame(spp=1, pipelined=1, **script(k)) for k in range(4)]      # fetch_image(lag=1): the stage adds no host synchronisation
    assert got[0] is None
    seq = [np.array(x) for x in got[1:]] + b.renderer.fetch_pending(all_images=True)
    assert len(seq) == 4
    for k in range(4):
        assert (_bits(seq[k]) == _bits(sync[k])).all(), k
    c = EarthViewer(**kw)
    assert c.renderer.local_exposure is None
    assert (_bits(c.frame(spp=1).copy()) != _bits(sync[0])).any()           # the frame loop did pick the setting up
    a.close(); b.close(); c.close()
