"""Bloom (include/digital_earth_bloom.h) on the GPU: the composited mean equals the numpy float32 restatement (tests/bloom_ref.py) bit for
bit on synthetic sums and from every source the display reads; the display is the unchanged transform over it; off is untouched; auto-exposure meters
the image before the bloom; the pipelined window loop; every error answers its code.

Sizes: a context's size is a multiple of (16, 8), so the two larger sizes are the nearest such sizes with the wanted properties.  16x8 has its levels
capped at 2.  80x56 has the levels 40x28, 20x14, 10x7, 5x4 and 3x2: odd widths and odd heights, five levels of the six asked for.  208x120 has several
workgroups per level and partial edge tiles at every level (104x60, 52x30, 26x15, 13x8, 7x4, 4x2).

Where the restatement's value is a NaN (only at a pixel whose own input holds one) the device must hold a NaN there; everything else is compared as bits."""
import ctypes

import numpy as np
import pytest

import bloom_ref as bl
import exposure_f64 as ae

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
SIZES = [(16, 8), (80, 56), (208, 120)]
SPPS = (1, 7)
TAUS = (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01)
SETTINGS = {
    "defaults": dict(),
    "threshold": dict(threshold=0.3, knee=0.5, clamp=2.0, intensity=0.4),
    "one level": dict(levels=1),
    "spread 0": dict(spread=0.0),
    "spread 1": dict(spread=1.0),
    "intensity 1": dict(intensity=1.0),
}


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


_INPUTS = {}


def _inputs(W, H):
    """name -> (W, H, 3) float32 sums, made once per size."""
    if (W, H) in _INPUTS:
        return _INPUTS[(W, H)]
    rng = np.random.default_rng(1000 * W + H)
    # log-uniform luminances over 2^-30 .. 2^10 with chroma in [-0.6, 2]: negative channels and negative luminances included
    mixed = (np.exp2(rng.uniform(-30.0, 10.0, (W, H, 1))) * rng.uniform(-0.6, 2.0, (W, H, 3))).astype(np.float32)
    # impulses at the four corners, on the four edges and in the interior, on black
    impulses = np.zeros((W, H, 3), np.float32)
    for k, (i, j) in enumerate([(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2 - 1, H - 1), (0, H // 2), (W - 1, H // 2 - 1),
                                (W // 2, H // 2), (W // 3, H // 3), (W // 3 + 1, H // 3)]):
        impulses[i, j] = (40.0 + k, 25.0 - k, 10.0 + 3 * k)
    constant = np.full((W, H, 3), 0.4, np.float32)
    zeros = np.zeros((W, H, 3), np.float32)
    # an ordinary scene with scattered pixels that are not light
    bright = (np.exp2(rng.uniform(-6.0, 3.0, (W, H, 1))) * rng.uniform(0.5, 1.5, (W, H, 3))).astype(np.float32)
    dirty = bright.copy()
    k = rng.permutation(W * H)[:max(W * H // 20, 6)]
    values = np.array([(np.nan, 1, 1), (np.inf, 1, 1), (-np.inf, 0, 0), (np.inf, -np.inf, 0), (1, np.nan, np.nan), (np.inf, np.inf, np.inf)], np.float32)
    dirty.reshape(-1, 3)[k] = values[np.arange(len(k)) % len(values)]
    _INPUTS[(W, H)] = dict(mixed=mixed, impulses=impulses, constant=constant, zeros=zeros, bright=bright, dirty=dirty)
    return _INPUTS[(W, H)]


# ---------------------------------------------------------------- 1. the composited mean, bit for bit
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("size", SIZES)
def test_bloom_hdr_equals_the_restatement_bit_for_bit(contexts, size, spp):
    W, H = size
    r = contexts(W, H)
    for name, sums in _inputs(W, H).items():
        r.upload_hdr(sums, spp)
        for setting, kw in SETTINGS.items():
            r.set_bloom(True, **kw)
            got = r.fetch_bloom_hdr()
            want, G, b = bl.bloom(sums, spp, **kw)
            _same(got, want, (name, setting))
            if name == "zeros":
                assert (_bits(got) == 0).all()
            if name == "constant" and kw.get("threshold", 0.0) == 0.0:
                assert (got == got[0, 0, 0]).all()                        # every pixel of every level sees the same values, clamped edges included
            if name == "impulses" and setting == "defaults":
                assert (G > 0).mean() > 0.2 and (got != bl.mean_of(sums, spp)).any()      # the glow did spread
    assert r.bloom() == dict(intensity=1.0, threshold=0.0, knee=0.5, clamp=0.0, spread=float(np.float32(0.7)), levels=6)
    r.set_bloom(False)
    assert r.bloom() is None


def test_levels_are_capped_by_the_image(contexts):
    """16x8 admits two levels: asking for 2, 6 or 10 gives the same bits, and 1 gives others."""
    r = contexts(16, 8)
    sums = _inputs(16, 8)["impulses"]
    r.upload_hdr(sums, 1)
    got = {}
    for levels in (1, 2, 6, 10):
        r.set_bloom(True, levels=levels)
        got[levels] = r.fetch_bloom_hdr()
    assert (_bits(got[2]) == _bits(got[6])).all() and (_bits(got[2]) == _bits(got[10])).all()
    assert (_bits(got[1]) != _bits(got[2])).any()
    r.set_bloom(False)


# ---------------------------------------------------------------- 2. the display is the unchanged transform over the composited mean
@pytest.mark.parametrize("size", SIZES)
def test_image_is_the_display_of_the_bloomed_mean(contexts, size):
    W, H = size
    r = contexts(W, H)
    for name, kw in (("bright", dict()), ("mixed", SETTINGS["threshold"]), ("impulses", dict(intensity=0.3))):
        sums = _inputs(W, H)[name]
        r.upload_hdr(sums, 3)
        r.set_bloom(True, **kw)
        on = r.fetch_image()
        mean = r.fetch_bloom_hdr()
        r.set_bloom(False)
        plain = r.fetch_image()
        r.upload_hdr(mean, 1)
        assert (_bits(r.fetch_image()) == _bits(on)).all(), name
        if name != "mixed":
            assert (_bits(plain) != _bits(on)).any(), name                # and the bloom shows


# ---------------------------------------------------------------- 3. off is untouched
def _rendered(R, seed=11):
    r = R.Renderer((64, 32), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=seed)
    r.copy_textures()
    r.accumulate(4)
    return r


def test_off_is_untouched(R):
    r = _rendered(R)
    hdr0 = r.fetch_hdr()
    before = r.fetch_image()
    assert r.bloom() is None
    r.set_bloom(True, intensity=0.5)
    on = r.fetch_image()
    assert (_bits(r.fetch_hdr()) == _bits(hdr0)).all()                    # the sums are never written
    _same(r.fetch_bloom_hdr(), bl.bloom(hdr0, 4, intensity=0.5)[0])
    assert (_bits(on) != _bits(before)).any()
    r.set_bloom(False)
    assert r.bloom() is None
    after = r.fetch_image()
    assert (_bits(after) == _bits(before)).all()
    assert (_bits(r.fetch_hdr()) == _bits(hdr0)).all()
    fresh = _rendered(R)
    assert (_bits(fresh.fetch_image()) == _bits(before)).all()
    fresh.close(); r.close()


# ---------------------------------------------------------------- 4. every display source
def test_bloom_reads_an_adaptive_frame_with_its_tile_counts(R):
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
    kw = dict(intensity=0.4, threshold=0.02)
    r.set_bloom(True, **kw)
    on = r.fetch_image()
    got = r.fetch_bloom_hdr()
    per_pixel = np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1)
    hdr = r.fetch_hdr()
    _same(got, bl.bloom(hdr, per_pixel, **kw)[0])
    assert (_bits(got) != _bits(bl.bloom(hdr, int(counts.max()), **kw)[0])).any()      # the frame's largest count would give something else
    r.set_bloom(False)
    r.reset_framebuffer()
    r.upload_hdr(got, 1)
    assert (_bits(r.fetch_image()) == _bits(on)).all()
    r.close()


def test_bloom_reads_the_denoised_mean(R):
    r = R.Renderer((64, 32), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=11)
    r.set_fov(0.42)
    r.copy_textures()
    r.set_denoise(True)
    kw = dict(intensity=0.4)
    r.set_bloom(True, **kw)
    r.reset_framebuffer()
    r.accumulate(4)
    on = r.fetch_image()
    got = r.fetch_bloom_hdr()
    filtered = r.fetch_denoised_hdr()
    _same(got, bl.bloom(filtered, 1, **kw)[0])
    assert (_bits(got) != _bits(bl.bloom(r.fetch_hdr(), 4, **kw)[0])).any()
    r.set_denoise(False)
    r.set_bloom(False)
    r.upload_hdr(got, 1)
    assert (_bits(r.fetch_image()) == _bits(on)).all()
    r.close()


@pytest.mark.parametrize("offset_floats", [0, 3])
def test_bloom_reads_a_display_source(R, offset_floats):
    """A second context's buffer as the display source; offset by one pixel (12 bytes) it is no longer 16-byte aligned: the scalar-load kernels."""
    W, H = 64, 32
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    other = R.Renderer((W, H + 8), (0, 1, 0), texture_source="constant")      # larger: the shifted window stays inside it
    r.copy_textures()
    rng = np.random.default_rng(5)
    big = (np.exp2(rng.uniform(-12.0, 4.0, (W, H + 8, 1))) * rng.uniform(0.2, 1.5, (W, H + 8, 3))).astype(np.float32)
    other.upload_hdr(big, 1)
    own = np.full((W, H, 3), 0.4, np.float32)
    r.upload_hdr(own, 5)
    ptr, _ = other.hdr_device_pointer()
    r.set_display_source(ptr + 4 * offset_floats)
    kw = dict(intensity=0.4, threshold=0.1)
    r.set_bloom(True, **kw)
    on = r.fetch_image()
    got = r.fetch_bloom_hdr()
    flat = np.ascontiguousarray(big.transpose(1, 0, 2)).ravel()              # the device layout [H][W][3]
    seen = flat[offset_floats:offset_floats + W * H * 3].reshape(H, W, 3).transpose(1, 0, 2)
    assert (_bits(r.fetch_hdr()) == _bits(seen)).all()
    _same(got, bl.bloom(seen, 5, **kw)[0])
    r.set_display_source(None)
    _same(r.fetch_bloom_hdr(), bl.bloom(own, 5, **kw)[0])
    r.set_bloom(False)
    r.upload_hdr(got, 1)
    assert (_bits(r.fetch_image()) == _bits(on)).all()
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
    big = (np.exp2(rng.uniform(-12.0, 4.0, (W, H + 8, 1))) * rng.uniform(0.2, 1.5, (W, H + 8, 3))).astype(np.float32)
    other.upload_hdr(big, 1)
    r.upload_hdr(np.full((W, H, 3), 0.4, np.float32), 3)
    yield r, other, np.ascontiguousarray(big.transpose(1, 0, 2)).ravel()      # the device layout [H][W][3]
    r.close(); other.close()


@pytest.mark.parametrize("offset_floats", [0, 1])
@pytest.mark.parametrize("levels", [1, 2, 10])
def test_pyramid_at_144x72(wide, levels, offset_floats):
    """The source aligned, and offset by one float (no longer 16-byte aligned: the scalar-load kernels)."""
    W, H = 144, 72
    r, other, flat = wide
    ptr, _ = other.hdr_device_pointer()
    kw = dict(intensity=0.4, threshold=0.1, levels=levels)
    assert bl.levels_used(W, H, levels) == min(levels, 6)
    r.set_display_source(ptr + 4 * offset_floats)
    r.set_bloom(True, **kw)
    got = r.fetch_bloom_hdr()
    seen = flat[offset_floats:offset_floats + W * H * 3].reshape(H, W, 3).transpose(1, 0, 2)
    r.set_bloom(False)
    r.set_display_source(None)
    _same(got, bl.bloom(seen, 3, **kw)[0])


# ---------------------------------------------------------------- 5. the scene is metered, not the lens
def test_auto_exposure_meters_the_image_before_the_bloom(contexts):
    W, H = 80, 56
    r = contexts(W, H)
    sums = _inputs(W, H)["bright"]
    kw = dict(intensity=0.5, threshold=0.2)
    manual = float(r.exposure[None])
    r.upload_hdr(sums, 3)
    r.set_auto_exposure(True)
    r.fetch_image()
    off = r.metering()
    r.set_auto_exposure(True)                       # clears the adaptation state, like the first time
    r.set_bloom(True, **kw)
    image = r.fetch_image()
    on = r.metering()
    assert on["ev"] == off["ev"] and on["ev_target"] == off["ev_target"] and on["mean_log2"] == off["mean_log2"] and on["valid"] and off["valid"]
    assert (on["histogram"] == off["histogram"]).all() and (on["metered"], on["below"], on["clipped"]) == (off["metered"], off["below"], off["clipped"])
    assert (on["histogram"] == ae.meter(sums, 3)["histogram"]).all()
    mean = r.fetch_bloom_hdr()
    _same(mean, bl.bloom(sums, 3, **kw)[0])
    r.set_auto_exposure(False)
    r.set_bloom(False)
    r.upload_hdr(mean, 1)
    r.set_exposure(on["ev"])
    assert (_bits(r.fetch_image()) == _bits(image)).all()
    r.set_exposure(manual)


# ---------------------------------------------------------------- 6. the pipelined window loop
def test_earth_viewer_frame_loop_pipelined_with_bloom():
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(64, 32), texture_source="synthetic", texture_size=(1024, 512), seed=5)

    def script(k):
        return dict(sun_angle=0.9) if k == 2 else {}

    def viewer(bloom=True):
        v = EarthViewer(**kw)
        if bloom:
            v.renderer.set_bloom(True, intensity=0.4)
        return v
    a = viewer()
    sync = [a.frame(spp=1, **script(k)).copy() for k in range(6)]
    b = viewer()
    got = [b.frame(spp=1, pipelined=2, **script(k)) for k in range(6)]
    assert got[0] is None and got[1] is None
    tail = b.renderer.fetch_pending(all_images=True)
    seq = [np.array(x) for x in got[2:]] + tail
    assert len(seq) == 6
    for k in range(6):
        assert (_bits(seq[k]) == _bits(sync[k])).all(), k
    assert b.finish() is None
    _same(b.renderer.fetch_bloom_hdr(), a.renderer.fetch_bloom_hdr())
    c = viewer(bloom=False)
    assert (_bits(c.frame(spp=1).copy()) != _bits(sync[0])).any()           # the frame loop did pick the setting up
    a.close(); b.close(); c.close()


# ---------------------------------------------------------------- 7. errors
def test_every_error_answers_its_code(contexts):
    from digital_earth_amd import _native
    W, H = 16, 8
    r = contexts(W, H)
    L, h = r._lib, r._h
    r.set_bloom(False)

    def settings(**kw):
        s = _native.DeBloom()
        s.struct_bytes = ctypes.sizeof(s)
        s.intensity, s.threshold, s.knee, s.clamp, s.spread, s.levels = 0.05, 0.0, 0.5, 0.0, 0.7, 6
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    out = np.empty((W, H, 3), np.float32)
    assert L.de_fetch_bloom_hdr(h, out.ctypes.data) == ERR_STATE              # off
    nan, inf = float("nan"), float("inf")
    bad = [dict(struct_bytes=24), dict(struct_bytes=32), dict(intensity=-0.1), dict(intensity=1.5), dict(intensity=nan), dict(threshold=-1.0), dict(threshold=nan),
           dict(threshold=inf), dict(knee=-0.1), dict(knee=1.5), dict(knee=nan), dict(clamp=-1.0), dict(clamp=nan), dict(clamp=inf), dict(spread=-0.1),
           dict(spread=1.5), dict(spread=nan), dict(levels=0), dict(levels=11), dict(levels=-3)]
    for kw in bad:
        assert L.de_set_bloom(h, ctypes.byref(settings(**kw))) == ERR_INVALID, kw
        assert r.bloom() is None                                              # a refused call changes nothing
    assert L.de_set_bloom(None, ctypes.byref(settings())) == ERR_INVALID
    assert L.de_get_bloom(h, None) == ERR_INVALID and L.de_fetch_bloom_hdr(h, None) == ERR_INVALID
    for kw in (dict(), dict(intensity=0.0), dict(intensity=1.0), dict(knee=0.0, threshold=2.0), dict(knee=1.0), dict(spread=0.0), dict(spread=1.0), dict(levels=1),
               dict(levels=10), dict(clamp=5.0)):
        assert L.de_set_bloom(h, ctypes.byref(settings(**kw))) == 0, kw
    r.upload_hdr(_inputs(W, H)["bright"], 2)
    assert L.de_fetch_bloom_hdr(h, out.ctypes.data) == 0
    assert L.de_set_bloom(h, None) == 0
    assert L.de_fetch_bloom_hdr(h, out.ctypes.data) == ERR_STATE
    got = _native.DeBloom()
    assert L.de_get_bloom(h, ctypes.byref(got)) == 0 and got.levels == 0 and got.struct_bytes == 28
