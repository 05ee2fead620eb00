"""The output scaling (include/digital_earth_output_scale.h) on the GPU: the two kernels equal the numpy restatement
(tests/output_scale_ref.py) bit for bit, on synthetic images through de_debug_output_scale and end to end behind the unchanged display transform and
ahead of the unchanged pack kernel; the library's tables meet the restatement's within a float32 ulp and sum to exactly one; the rings deliver the
synchronous bytes at the output size and re-allocate when it changes; a context that never touches the feature, or turns it off again, returns the
bytes it always returned; every error answers its code.

Size pairs (source -> output), the smallest at which each thing can go wrong:
    48 x 40 -> 32 x 24      non-integer shrink, a different ratio per axis
    16 x 8 -> 64 x 32       enlarging, every tap of the edge samples clamped
    64 x 64 -> 16 x 8       shrink by 4 and by 8: the most taps, and an LDS segment longer than a tile (64 outputs would read 512 pixels)
    80 x 56 -> 48 x 40      a partial tile on both axes
    48 x 40 -> 48 x 24      one axis a copy
    208 x 120 -> 112 x 72   several workgroups per axis (two tiles of 64 outputs along v, two chunks of 256 floats along u)"""
import ctypes

import numpy as np
import pytest

import output_scale_ref as ref
import pixels_ref as px

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = -1, -4
PAIRS = [((48, 40), (32, 24)), ((16, 8), (64, 32)), ((64, 64), (16, 8)), ((80, 56), (48, 40)), ((48, 40), (48, 24)), ((208, 120), (112, 72))]
# the special values of tests/test_gpu_pixels.py, thinned: -0.0, denormals, values below 0 and above 1, neighbours of 1 and of a k / 255 — and the non-finite ones
FINITE = np.array([-0.0, -1e-45, 1e-45, 1e-39, -1e-3, -2.0, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 1.5, 300.0, 128.0 / 255.0, 0.5, -3e38, 3e38], F)
NON_FINITE = np.array([np.nan, np.inf, -np.inf], F)


def images(W, H):
    """The (W, H, 3) inputs of the kernel test at one size: a ramp from below 0 to above 1 with the finite special values scattered in it, the same ramp
    with NaN and the infinities too (they spread over the filters' footprints; the rest of the image stays finite), and a random image in [0, 1]."""
    n = W * H * 3
    flat = np.arange(W * H, dtype=np.float64)[:, None]
    ramp = ((((flat * 0.37) % 258.0) - 1.0 + np.arange(3)[None, :] / 3.0) / 255.0).astype(F).ravel()
    a = ramp.copy()
    step = n // (len(FINITE) + 1)
    a[step // 2::step][:len(FINITE)] = FINITE
    b = a.copy()
    b[[n // 5 + 1, n // 2 + 2, (4 * n) // 5]] = NON_FINITE
    rng = np.random.default_rng(W * 1000 + H)
    return [a.reshape(W, H, 3), b.reshape(W, H, 3), rng.random((W, H, 3), dtype=F)]


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


def _same(got, want, what=""):
    """Bit for bit, NaN compared as NaN."""
    assert got.dtype == F and got.shape == want.shape, (what, got.shape, want.shape)
    diff = ~((_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want)))
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def _equal(got, want, what=""):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    diff = got != want
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def _sums(W, H, seed=0):
    """Sums whose display covers black, mid greys and clipped white (tests/test_gpu_pixels.py)."""
    rng = np.random.default_rng(100 * W + H + seed)
    s = (np.exp2(rng.uniform(-9.0, 3.0, (W, H, 1))) * rng.uniform(0.3, 1.6, (W, H, 3))).astype(F)
    s[: W // 4, : H // 4] = 0.0
    return s


def _tables(r, src, dst, filter):
    """The library's own tables for (W, H) -> (ow, oh): the image comparison is then independent of libm."""
    (W, H), (ow, oh) = src, dst
    return (r.debug_output_scale_weights(W, ow, filter) if ow != W else None, r.debug_output_scale_weights(H, oh, filter) if oh != H else None)


def _resampled(r, image, size, filter):
    return ref.resample(image, size, filter, tables=_tables(r, image.shape[:2], size, filter))


OFF = dict(filter="lanczos3", on=False)


# ---------------------------------------------------------------- 1. the kernels, bit for bit
@pytest.mark.parametrize("pair", PAIRS)
def test_kernel_equals_the_restatement_bit_for_bit(contexts, pair):
    src, dst = pair
    r = contexts(16, 8)                                       # de_debug_output_scale is free of the context's size
    held = r.output_scale()
    for filter in ref.FILTERS:
        tables = _tables(r, src, dst, filter)
        wants = []
        for n, img in enumerate(images(*src)):
            got = r.debug_output_scale(img, dst, filter)
            wants.append(ref.resample(img, dst, filter, tables=tables))
            _same(got, wants[n], (filter, n))
            assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0 and not np.signbit(got).any()      # the last pass clamps: NaN gives 0
        assert 3 <= int((_bits(wants[0]) != _bits(wants[1])).sum()) < wants[0].size      # NaN and the infinities reached their footprints, and not everything
        _same(r.debug_output_scale(images(*src)[1], src, filter), images(*src)[1], filter)      # the same size: the identity, NaN and -0.0 included
    assert r.output_scale() == held and r.output_size() == (16, 8)      # the debug entry point leaves the context's setting alone


# ---------------------------------------------------------------- 2. the tables
@pytest.mark.parametrize("filter", ref.FILTERS)
def test_tables_meet_the_restatement_and_sum_to_exactly_one(contexts, filter):
    r = contexts(16, 8)
    axes = sorted({(s[k], d[k]) for s, d in PAIRS for k in (0, 1) if s[k] != d[k]} | {(2160, 1080), (544, 1080), (64, 8), (8, 64)})
    for n_src, n_dst in axes:
        first, w = r.debug_output_scale_weights(n_src, n_dst, filter)
        want_first, want_w = ref.weights(n_src, n_dst, filter)
        assert first.dtype == np.int32 and (first == want_first).all() and w.shape == want_w.shape, (n_src, n_dst)
        assert w.shape[1] <= ref.MAX_TAPS
        assert (_bits(ref.row_sums(w)) == _bits(F(1.0))).all(), (n_src, n_dst)      # the exact-one property, of the library's own table
        # Two libms evaluate the Lanczos sine: every tap within one float32 ulp of the row's largest weight — but for the row's last tap, which the
        # correction makes 1 minus the float32 sum of the others: it may move by the ulps of all of them together.
        cnt = np.array(ref.geometry(n_src, n_dst, filter)[4])
        ulp = np.spacing(np.abs(want_w).max(axis=1).astype(F)).astype(np.float64)
        err = np.abs(w.astype(np.float64) - want_w.astype(np.float64))
        last = np.arange(w.shape[1])[None, :] == (cnt - 1)[:, None]
        assert (err <= np.where(last, cnt[:, None] * ulp[:, None], ulp[:, None])).all(), (n_src, n_dst)
    assert r._lib.de_debug_output_scale_weights(r._h, 8, 72, 0, None, None, ctypes.byref(ctypes.c_int())) == ERR_INVALID       # ratio 9
    assert r._lib.de_debug_output_scale_weights(r._h, 64, 32, 4, None, None, ctypes.byref(ctypes.c_int())) == ERR_INVALID      # no such filter


# ---------------------------------------------------------------- 3. end to end behind the display
@pytest.mark.parametrize("case", [((64, 32), ((48, 24), (128, 40))), ((80, 56), ((48, 40), (112, 72)))])
def test_fetches_deliver_the_restatement_of_the_displayed_image(R, contexts, case):
    (W, H), sizes = case
    r = contexts(W, H)
    sums = _sums(W, H)
    never = R.Renderer((W, H), (0, 1, 0), texture_source="constant")      # the feature is never touched on this one
    never.copy_textures()
    never.upload_hdr(sums, 3)
    r.upload_hdr(sums, 3)
    before = r.fetch_image()
    before_px = r.fetch_pixels()
    assert before.shape == (W, H, 3) and r.output_size() == (W, H)
    assert len(np.unique(px.pack(before, 3))) > 16             # a picture, not a flat field
    for size in sizes:
        for filter in ref.FILTERS:
            r.set_output_scale(size, filter)
            assert r.output_size() == size and r.output_scale() == dict(size=size, filter=filter, on=True)
            want = _resampled(r, before, size, filter)
            _same(r.fetch_image(), want, (size, filter))
            view = r.fetch_image(copy=False)
            _same(np.array(view), want, (size, filter, "view"))
            del view
            for channels, mode in ((4, "truncate"), (3, "round"), (3, "dither")):
                r.set_pixels(channels, mode, seed=5)
                got = r.fetch_pixels()
                assert got.shape == (size[1], size[0], channels)
                _equal(got, px.pack(want, channels, mode, 5, 0), (size, filter, channels, mode))
            r.set_pixels()
            assert (_bits(r.fetch_hdr()) == _bits(never.fetch_hdr())).all()          # (W, H, 3) through the shared staging buffer
    # on at the context's own size: the identity, bit for bit, for every filter
    for filter in ref.FILTERS:
        r.set_output_scale(None, filter)
        assert r.output_size() == (W, H)
        _same(r.fetch_image(), before, filter)
    # the context that never touched the feature, and this one after turning it off, return the bytes they always returned
    assert (_bits(never.fetch_image()) == _bits(before)).all()
    _equal(never.fetch_pixels(), before_px)
    r.set_output_scale(sizes[0], "mitchell")
    r.set_output_scale(on=False)
    assert r.output_size() == (W, H) and r.output_scale()["on"] is False
    assert (_bits(r.fetch_image()) == _bits(before)).all()
    _equal(r.fetch_pixels(), before_px)
    view = r.fetch_image(copy=False)
    assert view.shape == (W, H, 3) and (_bits(np.array(view)) == _bits(before)).all()
    del view
    never.close()


def test_black_and_clipped_white_survive_every_scale(contexts):
    r = contexts(16, 8)
    for src, dst in PAIRS:
        for filter in ref.FILTERS:
            for value in (0.0, 1.0):
                got = r.debug_output_scale(np.full(src + (3,), value, F), dst, filter)
                assert (_bits(got) == _bits(F(value))).all(), (src, dst, filter, value)


# ---------------------------------------------------------------- 4. rings
def _frames(W, H, n):
    return [_sums(W, H, seed=k + 1) for k in range(n)]


@pytest.mark.parametrize("lag", (1, 2, 3))
def test_lagged_fetches_give_the_synchronous_bytes_at_the_output_size(contexts, lag):
    W, H = 80, 56
    size = (112, 40)                                          # enlarged along u, shrunk along v
    r = contexts(W, H)
    frames = _frames(W, H, 5)
    r.set_output_scale(size, "lanczos3")
    r.set_pixels(3, "round")
    sync_f, sync_p = [], []
    for s in frames:
        r.upload_hdr(s, 2)
        sync_f.append(r.fetch_image())
        sync_p.append(r.fetch_pixels())
    assert sync_f[0].shape == size + (3,) and sync_p[0].shape == (size[1], size[0], 3)
    got_f, got_p = [], []
    for s in frames:                                          # both rings at once: they stay independent
        r.upload_hdr(s, 2)
        got_f.append(r.fetch_image(lag=lag))
        got_p.append(r.fetch_pixels(lag=lag))
    assert all(g is None for g in got_f[:lag] + got_p[:lag])
    with pytest.raises(Exception) as e:
        r.set_output_scale((48, 24))                          # refused while fetches are in flight
    assert e.value.code == ERR_STATE and r.output_size() == size
    tail_p = r.fetch_pending(all_images=True, pixels=True)
    with pytest.raises(Exception) as e:
        r.set_output_scale((48, 24))                          # the float ring alone refuses too
    assert e.value.code == ERR_STATE and r.output_size() == size
    tail_f = r.fetch_pending(all_images=True)
    seq_f, seq_p = got_f[lag:] + tail_f, got_p[lag:] + tail_p
    assert len(tail_f) == lag and len(tail_p) == lag and len(seq_f) == len(frames) == len(seq_p)
    for k in range(len(frames)):
        _same(seq_f[k], sync_f[k], k)
        _equal(seq_p[k], sync_p[k], k)
    r.set_pixels()
    r.set_output_scale(**OFF)


def test_a_change_of_size_reallocates_larger_then_smaller(contexts):
    W, H = 64, 32
    r = contexts(W, H)
    r.upload_hdr(_sums(W, H, 7), 2)
    base = r.fetch_image()
    r.fetch_image(copy=False); r.fetch_pixels(copy=False)      # the staging buffers exist at W x H
    for k in range(4):                                        # and so do all the ring cells
        r.fetch_image(lag=1); r.fetch_pixels(lag=1)
    r.fetch_pending(); r.fetch_pending(pixels=True)
    for size in ((256, 128), (16, 8), (128, 64), (64, 32)):   # larger, smaller, larger again, the context's own
        r.set_output_scale(size, "triangle")
        want = _resampled(r, base, size, "triangle")
        _same(r.fetch_image(), want, size)
        _same(np.array(r.fetch_image(copy=False)), want, size)
        _equal(r.fetch_pixels(), px.pack(want), size)
        _equal(np.array(r.fetch_pixels(copy=False)), px.pack(want), size)
        got = [r.fetch_image(lag=2) for k in range(5)] + r.fetch_pending(all_images=True)
        assert [g is None for g in got] == [True, True] + [False] * 5
        for g in got[2:]:
            _same(g, want, size)
        gotp = [r.fetch_pixels(lag=3) for k in range(6)] + r.fetch_pending(all_images=True, pixels=True)
        for g in gotp[3:]:
            _equal(g, px.pack(want), size)
        assert (_bits(r.fetch_hdr()).shape == (W, H, 3))
    r.set_output_scale(**OFF)
    _same(r.fetch_image(), base)


# ---------------------------------------------------------------- 5. errors
def test_every_error_answers_its_code(contexts):
    from digital_earth_amd import _native
    W, H = 64, 32
    r = contexts(W, H)
    L, h = r._lib, r._h

    def settings(**kw):
        s = _native.DeOutputScale()
        s.struct_bytes, s.enabled, s.width, s.height, s.filter = ctypes.sizeof(s), 1, 32, 16, 3
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    r.set_output_scale((128, 24), "mitchell")
    held = r.output_scale()
    bad = (dict(width=40), dict(height=12), dict(width=0), dict(height=0), dict(width=-32), dict(width=528), dict(height=264), dict(height=-8), dict(width=4), dict(filter=-1), dict(filter=4), dict(struct_bytes=16), dict(struct_bytes=24), dict(width=520), dict(height=4))
    for kw in bad:
        assert L.de_set_output_scale(h, ctypes.byref(settings(**kw))) == ERR_INVALID, kw
        assert r.output_scale() == held and r.output_size() == (128, 24)      # a refused call changes nothing
    assert L.de_set_output_scale(h, ctypes.byref(settings(width=512, height=256))) == 0 and r.output_size() == (512, 256)      # ratio 8: the bound itself
    assert L.de_set_output_scale(h, ctypes.byref(settings(width=16, height=8))) == 0 and r.output_size() == (16, 8)            # ratio 1/4 and 1/4
    assert L.de_set_output_scale(h, ctypes.byref(settings(enabled=0, width=40))) == ERR_INVALID                                # the size is checked while off too
    r.set_output_scale((128, 24), "mitchell")
    assert L.de_set_output_scale(h, None) == ERR_INVALID and L.de_set_output_scale(None, ctypes.byref(settings())) == ERR_INVALID
    assert L.de_get_output_scale(h, None) == ERR_INVALID and L.de_output_size(h, None, None) == ERR_INVALID
    got = _native.DeOutputScale()
    assert L.de_get_output_scale(h, ctypes.byref(got)) == 0 and (got.struct_bytes, got.enabled, got.width, got.height, got.filter) == (20, 1, 128, 24, 2)
    # a set while a float fetch is in flight, and while a pixel fetch is
    r.upload_hdr(_sums(W, H), 1)
    assert L.de_fetch_image_begin(h) == 0
    assert L.de_set_output_scale(h, ctypes.byref(settings())) == ERR_STATE and r.output_scale() == held
    fp, bp = ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_uint8)()
    assert L.de_fetch_image_end(h, ctypes.byref(fp)) == 0
    assert L.de_fetch_pixels_begin(h) == 0
    assert L.de_set_output_scale(h, ctypes.byref(settings())) == ERR_STATE and r.output_scale() == held
    assert L.de_fetch_pixels_end(h, ctypes.byref(bp)) == 0
    assert L.de_set_output_scale(h, ctypes.byref(settings())) == 0 and r.output_size() == (32, 16)
    # the debug entry point checks the same rules against the image's size
    img, out = np.zeros((W, H, 3), F), np.empty((512, 256, 3), F)
    for kw in (dict(width=40), dict(height=12), dict(width=528), dict(width=4, height=8), dict(filter=4), dict(struct_bytes=16)):
        assert L.de_debug_output_scale(h, img.ctypes.data, W, H, ctypes.byref(settings(**kw)), out.ctypes.data) == ERR_INVALID, kw
    assert L.de_debug_output_scale(h, img.ctypes.data, 24, 8, ctypes.byref(settings()), out.ctypes.data) == ERR_INVALID      # W not a multiple of 16
    assert L.de_debug_output_scale(h, None, W, H, ctypes.byref(settings()), out.ctypes.data) == ERR_INVALID
    wide = np.zeros((144, 8, 3), F)
    assert L.de_debug_output_scale(h, wide.ctypes.data, 144, 8, ctypes.byref(settings(width=16, height=8)), out.ctypes.data) == ERR_INVALID      # ratio 1/9
    with pytest.raises(ValueError):
        r.set_output_scale((32, 16), filter="bicubic")
    r.set_output_scale(**OFF)
    assert r.output_scale() == dict(size=(W, H), filter="lanczos3", on=False) and r.output_size() == (W, H)


# ---------------------------------------------------------------- 6. the viewer
def test_earth_viewer_frames_and_saves_at_the_output_size(tmp_path):
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(64, 32), texture_source="synthetic", texture_size=(1024, 512), seed=5)
    a, b = EarthViewer(**kw), EarthViewer(output_res=(32, 16), output_filter="mitchell", **kw)
    assert b.renderer.output_scale() == dict(size=(32, 16), filter="mitchell", on=True) and a.renderer.output_size() == (64, 32)
    full = [a.frame(spp=1).copy() for k in range(3)]
    got = [b.frame(spp=1).copy() for k in range(3)]
    for k in range(3):
        _same(got[k], _resampled(b.renderer, full[k], (32, 16), "mitchell"), k)
    pix = b.frame(spp=1, pixels=True)
    assert pix.shape == (16, 32, 4)
    b.save(str(tmp_path / "b.npy"))
    assert np.load(str(tmp_path / "b.npy")).shape == (32, 16, 3)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:      # only this check needs PIL
        b.save(str(tmp_path / "b.png"))                       # the picture of the last frame(pixels=True)
        decoded = np.array(Image.open(str(tmp_path / "b.png")))
        assert decoded.shape == (16, 32, 3) and (decoded == pix[..., :3]).all()
        c = EarthViewer(output_res=(128, 64), **kw)
        shown = c.render(spp=1).copy()
        assert shown.shape == (128, 64, 3)
        c.save(str(tmp_path / "c.png"))                       # the held float image through the pack kernel, at the output size
        assert (np.array(Image.open(str(tmp_path / "c.png"))) == px.pack(shown, 3)).all()
        c.close()
    a.close(); b.close()
