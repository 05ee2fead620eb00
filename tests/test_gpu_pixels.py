"""The 8-bit pixel output (include/digital_earth_pixels.h) on the GPU: the bytes of pixels_pack_kernel equal the numpy restatement
(tests/pixels_ref.py) exactly, on synthetic images through de_debug_pixels and end to end behind the unchanged display transform; the float image is
untouched; the pixel ring is pipelined and independent of the float ring; every error answers its code.

Sizes: 16x8 is one partial workgroup (half a tile wide, a quarter high), 80x56 is ragged in both directions (2.5 x 1.75 tiles), 208x120 has several
workgroups with ragged edges (6.5 x 3.75 tiles)."""
import ctypes

import numpy as np
import pytest

import pixels_ref as px

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = -1, -4
SIZES = [(16, 8), (80, 56), (208, 120)]
PHASES = (0, 1, 77)


def special_values():
    """Every k/255 with its two f32 neighbours, values below 0 and above 1, -0.0, the infinities and NaN."""
    k = np.arange(256, dtype=F) / F(255.0)
    return np.concatenate([np.nextafter(k, F(-np.inf)), k, np.nextafter(k, F(np.inf)),
                           np.array([-0.0, -1e-45, -1e-3, -2.0, -3e38, 1.0 + 2.0 ** -23, 1.5, 300.0, 3e38, np.inf, -np.inf, np.nan, 1e-45, 0.5], F)]).astype(F)


def images(W, H):
    """The (W, H, 3) inputs of the kernel test at one size.  Every image is a slow ramp — 1/8 LSB per pixel along the columns, a third of an LSB between
    the channels, running from below 0 to above 255 so that both ends of the dither's fade are crossed — with the special values at its odd flat
    indices, as many as fit; the small size takes several images to hold them all."""
    n = W * H * 3
    sp = special_values()
    flat = np.arange(W * H, dtype=np.float64)[:, None]
    ramp = ((((flat / 8.0) % 258.0) - 1.0 + np.arange(3)[None, :] / 3.0) / 255.0).astype(F).ravel()
    per = min(len(sp), n // 2)
    out = []
    for start in range(0, len(sp), per):
        chunk = sp[start:start + per]
        img = ramp.copy()
        img[1:2 * len(chunk):2] = chunk
        out.append(img.reshape(W, H, 3))
    return out


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
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _equal(got, want, what=""):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    diff = got != want
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def _sums(W, H, seed=0):
    """Sums whose display covers black, mid greys and clipped white."""
    rng = np.random.default_rng(100 * W + H + seed)
    s = (np.exp2(rng.uniform(-9.0, 3.0, (W, H, 1))) * rng.uniform(0.3, 1.6, (W, H, 3))).astype(F)
    s[: W // 4, : H // 4] = 0.0
    return s


# ---------------------------------------------------------------- 1. the kernel, byte for byte
@pytest.mark.parametrize("size", SIZES)
def test_kernel_equals_the_restatement_byte_for_byte(contexts, size):
    W, H = size
    r = contexts(16, 8)                                       # de_debug_pixels is free of the context's size
    seen = set()
    for n, img in enumerate(images(W, H)):
        for channels in (3, 4):
            for mode in px.MODES:
                for phase in PHASES:
                    seed = 0 if phase == 0 else 0xC0FFEE + phase
                    got = r.debug_pixels(img, channels=channels, mode=mode, seed=seed, phase=phase)
                    want = px.pack(img, channels, mode, seed, phase)
                    _equal(got, want, (n, channels, mode, phase))
                    if channels == 4:
                        assert (got[..., 3] == 255).all()
                    seen.add(bytes(got[..., :3]))
    assert len(seen) == 5 * len(images(W, H))                 # per image: truncate, round (both ignore the phase) and one dither per phase
    assert r.pixels() == dict(px.DEFAULTS, last_phase=0)      # the debug entry point leaves the context's settings and counter alone


# ---------------------------------------------------------------- 2. end to end behind the display
@pytest.mark.parametrize("size", SIZES)
def test_fetch_pixels_is_the_restatement_of_fetch_image(R, contexts, size):
    W, H = size
    r = contexts(W, H)
    sums = _sums(W, H)
    never = R.Renderer((W, H), (0, 1, 0), texture_source="constant")      # the feature is never touched on this one
    never.copy_textures()
    never.upload_hdr(sums, 3)
    r.upload_hdr(sums, 3)
    before = r.fetch_image()
    assert (_bits(before) == _bits(never.fetch_image())).all()
    assert len(np.unique(px.pack(before, 3))) > 16             # a picture, not a flat field
    for channels in (4, 3):
        for mode in px.MODES:
            r.set_pixels(channels, mode, seed=5)
            _equal(r.fetch_pixels(), px.pack(before, channels, mode, 5, 0), (channels, mode))
            assert r.pixels() == dict(channels=channels, mode=mode, seed=5, animate=False, last_phase=0)
            view = r.fetch_pixels(copy=False)
            _equal(np.array(view), px.pack(before, channels, mode, 5, 0))
            del view
    # with bloom and auto-exposure on: whatever the display honours is inherited
    for x in (r, never):
        x.set_bloom(True, intensity=0.4)
        x.set_auto_exposure(True)
    shown = r.fetch_image()
    assert (_bits(shown) != _bits(before)).any()
    r.set_pixels(3, "dither", seed=8)
    _equal(r.fetch_pixels(), px.pack(shown, 3, "dither", 8, 0))
    assert (_bits(r.fetch_image()) == _bits(shown)).all() and (_bits(never.fetch_image()) == _bits(shown)).all()
    for x in (r, never):
        x.set_bloom(False)
        x.set_auto_exposure(False)
    after = r.fetch_image()
    assert (_bits(after) == _bits(before)).all() and (_bits(never.fetch_image()) == _bits(before)).all()
    assert (_bits(r.fetch_hdr()) == _bits(never.fetch_hdr())).all()
    r.set_pixels()
    never.close()


def test_fetch_pixels_reads_an_adaptive_frame_with_its_tile_counts(R):
    r = R.Renderer((64, 32), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=11)
    r.set_fov(0.42)
    r.copy_textures()
    for tau in (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01):
        r.reset_framebuffer()
        r.render_adaptive(tau, 32, min_spp=4, round_spp=4)
        if len(np.unique(r.tile_spp())) >= 2:
            break
    else:
        pytest.fail("no threshold spreads the tile counts")
    image = r.fetch_image()
    for channels, mode in ((4, "truncate"), (3, "dither")):
        r.set_pixels(channels, mode, seed=3)
        _equal(r.fetch_pixels(), px.pack(image, channels, mode, 3, 0))
    assert (_bits(r.fetch_image()) == _bits(image)).all()
    r.close()


# ---------------------------------------------------------------- 3. pipelined fetches
def _frames(W, H, n):
    return [_sums(W, H, seed=k + 1) for k in range(n)]


@pytest.mark.parametrize("lag", (1, 2, 3))
def test_lagged_fetches_give_the_synchronous_bytes(contexts, lag):
    W, H = 80, 56
    r = contexts(W, H)
    frames = _frames(W, H, 6)
    r.set_pixels(3, "dither", seed=21, animate=True)
    sync = []
    for k, s in enumerate(frames):
        r.upload_hdr(s, 2)
        sync.append(r.fetch_pixels())
        assert r.pixels()["last_phase"] == k                  # the phase advances by one per conversion
    for k, s in enumerate(frames):                            # the phases are part of the bytes
        _equal(sync[k], px.pack(_display(r, s), 3, "dither", 21, k), k)
    r.set_pixels(3, "dither", seed=21, animate=True)          # resets the counter
    got = []
    for k, s in enumerate(frames):
        r.upload_hdr(s, 2)
        got.append(r.fetch_pixels(lag=lag))
        assert r.pixels()["last_phase"] == k
    assert all(g is None for g in got[:lag])
    with pytest.raises(RuntimeError):
        r.fetch_pixels()                                      # lagged fetches are in flight
    assert r.fetch_pending() is None                          # the float ring has nothing, and the pixel ring is left alone
    tail = r.fetch_pending(all_images=True, pixels=True)
    seq = got[lag:] + tail
    assert len(tail) == lag and len(seq) == len(frames) and r.fetch_pending(pixels=True) is None
    for k in range(len(frames)):
        _equal(seq[k], sync[k], k)
    r.set_pixels()


def _display(r, sums):
    r.upload_hdr(sums, 2)
    return r.fetch_image()


def test_float_and_pixel_rings_are_independent(contexts):
    from digital_earth_amd import _native
    W, H = 80, 56
    r = contexts(W, H)
    L, h = r._lib, r._h
    frames = _frames(W, H, 8)
    r.set_pixels(4, "round")
    images = [_display(r, s) for s in frames]
    # interleaved: float begins on frames 0, 2, 4, 6, pixel begins on frames 1, 3, 5, 7
    for k, s in enumerate(frames):
        r.upload_hdr(s, 2)
        assert (L.de_fetch_image_begin(h) if k % 2 == 0 else L.de_fetch_pixels_begin(h)) == 0
    assert L.de_fetch_pixels_begin(h) == ERR_STATE            # the fifth
    assert L.de_fetch_image_begin(h) == ERR_STATE
    s = _native.DePixels()
    s.struct_bytes, s.channels, s.mode = ctypes.sizeof(s), 3, 0
    assert L.de_set_pixels(h, ctypes.byref(s)) == ERR_STATE   # while pixel fetches are in flight
    assert r.pixels()["channels"] == 4
    fp, bp = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_uint8)()
    for k in (1, 0, 3, 2, 5, 7, 4, 6):                        # any order of the two rings: each hands out its own oldest
        if k % 2 == 0:
            assert L.de_fetch_image_end(h, ctypes.byref(fp)) == 0
            assert (_bits(np.ctypeslib.as_array(fp, shape=(W, H, 3))) == _bits(images[k])).all(), k
        else:
            assert L.de_fetch_pixels_end(h, ctypes.byref(bp)) == 0
            _equal(np.ctypeslib.as_array(bp, shape=(H, W, 4)).copy(), px.pack(images[k], 4, "round"), k)
    assert L.de_fetch_pixels_end(h, ctypes.byref(bp)) == ERR_STATE and L.de_fetch_image_end(h, ctypes.byref(fp)) == ERR_STATE
    assert L.de_set_pixels(h, ctypes.byref(s)) == 0 and r.pixels()["channels"] == 3
    r.set_pixels()


# ---------------------------------------------------------------- 4. errors, views, the viewer
def test_every_error_answers_its_code(contexts):
    from digital_earth_amd import _native
    W, H = 16, 8
    r = contexts(W, H)
    L, h = r._lib, r._h

    def settings(**kw):
        s = _native.DePixels()
        s.struct_bytes, s.channels, s.mode, s.seed, s.animate = ctypes.sizeof(s), 4, 0, 0, 0
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    r.set_pixels(3, "round", seed=4, animate=True)
    held = r.pixels()
    for kw in (dict(struct_bytes=16), dict(struct_bytes=24), dict(channels=0), dict(channels=2), dict(channels=5), dict(channels=-3), dict(mode=-1), dict(mode=3)):
        assert L.de_set_pixels(h, ctypes.byref(settings(**kw))) == ERR_INVALID, kw
        assert r.pixels() == held                             # a refused call changes nothing
    assert L.de_set_pixels(h, None) == ERR_INVALID and L.de_set_pixels(None, ctypes.byref(settings())) == ERR_INVALID
    assert L.de_get_pixels(h, None, None) == ERR_INVALID
    got = _native.DePixels()
    assert L.de_get_pixels(h, ctypes.byref(got), None) == 0 and (got.struct_bytes, got.channels, got.mode, got.seed, got.animate) == (20, 3, 1, 4, 1)
    r.upload_hdr(_sums(W, H), 1)
    out = np.empty((H, W, 3), np.uint8)
    assert L.de_fetch_pixels(h, out.ctypes.data, ctypes.c_uint64(out.nbytes - 1)) == ERR_INVALID
    assert L.de_fetch_pixels(h, None, ctypes.c_uint64(out.nbytes)) == ERR_INVALID
    assert L.de_fetch_pixels(h, out.ctypes.data, ctypes.c_uint64(out.nbytes)) == 0
    assert L.de_fetch_pixels_view(h, None) == ERR_INVALID and L.de_fetch_pixels_end(h, None) == ERR_INVALID
    img = np.zeros((W, H, 3), F)
    for kw in (dict(struct_bytes=16), dict(channels=2), dict(mode=3)):
        assert L.de_debug_pixels(h, img.ctypes.data, W, H, ctypes.byref(settings(**kw)), 0, out.ctypes.data) == ERR_INVALID, kw
    assert L.de_debug_pixels(h, img.ctypes.data, 24, 8, ctypes.byref(settings()), 0, out.ctypes.data) == ERR_INVALID      # W not a multiple of 16
    assert L.de_debug_pixels(h, img.ctypes.data, 16, 4, ctypes.byref(settings()), 0, out.ctypes.data) == ERR_INVALID      # H not a multiple of 8
    with pytest.raises(ValueError):
        r.set_pixels(mode="blue noise")
    with pytest.raises(ValueError):
        r.fetch_pixels(lag=4)
    r.set_pixels()
    assert r.pixels() == dict(px.DEFAULTS, last_phase=0)


def test_a_view_lives_until_the_next_pixel_fetch_and_holds_the_renderer(R):
    W, H = 16, 8
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    r.copy_textures()
    a, b = _sums(W, H, 1), _sums(W, H, 2)
    r.upload_hdr(a, 1)
    want_a = px.pack(r.fetch_image(), 4)
    view = r.fetch_pixels(copy=False)
    assert view.shape == (H, W, 4) and not view.flags.writeable
    r.fetch_image(); r.fetch_image(copy=False); r.fetch_hdr()          # float fetches use other buffers
    _equal(np.array(view), want_a)
    r.upload_hdr(b, 1)
    view2 = r.fetch_pixels(copy=False)                                  # the next pixel fetch overwrites it
    _equal(np.array(view), px.pack(r.fetch_image(), 4))
    del view
    with pytest.raises(RuntimeError):
        r.close()
    del view2
    r.close()


def test_earth_viewer_frames_and_saves_pixels(tmp_path):
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(64, 32), texture_source="synthetic", texture_size=(1024, 512), seed=5)
    a, b, c = EarthViewer(**kw), EarthViewer(**kw), EarthViewer(**kw)
    floats = [a.frame(spp=1).copy() for k in range(4)]
    got = [b.frame(spp=1, pixels=True) for k in range(4)]
    for k in range(4):
        _equal(got[k], px.pack(floats[k]), k)
    piped = [c.frame(spp=1, pipelined=2, pixels=True) for k in range(4)]
    assert piped[0] is None and piped[1] is None
    _equal(piped[2], px.pack(floats[0]))
    _equal(c.finish(pixels=True), px.pack(floats[3]))
    assert c.finish(pixels=True) is None and c.finish() is None
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:      # only this check needs PIL
        old = (np.clip(floats[3], 0.0, 1.0) * 255).astype(np.uint8).transpose(1, 0, 2)[::-1]      # the previous save()'s expression
        a.save(str(tmp_path / "a.png"))
        decoded = np.array(Image.open(str(tmp_path / "a.png")))
        assert decoded.shape == old.shape and (decoded == old).all()
        Image.fromarray(old).save(str(tmp_path / "old.png"))
        assert (tmp_path / "a.png").read_bytes() == (tmp_path / "old.png").read_bytes()
        b.save(str(tmp_path / "b.png"))                                   # the picture of the last frame(pixels=True)
        assert (np.array(Image.open(str(tmp_path / "b.png"))) == old).all()
    a.close(); b.close(); c.close()


def test_save_writes_the_picture_shown_not_a_new_display(tmp_path):
    """A display-only slider changed by frame() (written to the renderer after the fetch, no reset), bloom turned on or the exposure set directly after
    the picture was fetched must not reach the file: save() writes what frame() returned, as the previous expression did."""
    Image = pytest.importorskip("PIL.Image")
    from digital_earth_amd.earth_viewer import EarthViewer
    v = EarthViewer(screen_res=(64, 32), texture_source="synthetic", texture_size=(1024, 512), seed=5)
    v.frame(spp=2)
    shown = v.frame(spp=1, exposure=float(v.renderer.exposure[None]) + 2.0, gamma=1.7).copy()
    old = (np.clip(shown, 0.0, 1.0) * 255).astype(np.uint8).transpose(1, 0, 2)[::-1]
    moved = v.renderer.fetch_image()
    assert (px.pack(moved, 3) != old).any()                               # the context would display something else now
    for channels in (4, 3):
        v.renderer.set_pixels(channels)
        v.save(str(tmp_path / "s.png"))
        decoded = np.array(Image.open(str(tmp_path / "s.png")))
        assert decoded.shape == old.shape and (decoded == old).all()
    Image.fromarray(old).save(str(tmp_path / "old.png"))
    assert (tmp_path / "s.png").read_bytes() == (tmp_path / "old.png").read_bytes()
    w = EarthViewer(screen_res=(64, 32), texture_source="synthetic", texture_size=(1024, 512), seed=5)
    img = w.render(spp=2).copy()
    w.renderer.set_bloom(True, intensity=0.5)
    w.renderer.exposure[None] = float(w.renderer.exposure[None]) + 1.0
    w.save(str(tmp_path / "w.png"))
    assert (np.array(Image.open(str(tmp_path / "w.png"))) == (np.clip(img, 0.0, 1.0) * 255).astype(np.uint8).transpose(1, 0, 2)[::-1]).all()
    w.renderer.set_pixels(3, "round")                                     # the renderer's current mode is honoured
    w.save(str(tmp_path / "w.png"))
    assert (np.array(Image.open(str(tmp_path / "w.png"))) == px.pack(img, 3, "round")).all()
    v.close(); w.close()
