"""The video frame output (include/digital_earth_video.h) on the GPU: the bytes of videoframe_pack_kernel equal the numpy restatement
(tests/video_ref.py) exactly, on synthetic images through de_debug_video and end to end behind the unchanged display transform, output scaling and the
HDR signal; the other fetches are untouched; the video ring is pipelined and independent of the float and pixel rings; every error answers its code.

Sizes: 16x8 is one partial workgroup; 18x10 has a width of 2 mod 4 (an odd chroma stride: the narrow stores of NV12, I420 and I010); 20x6 a width of
4 mod 8 (I420: Y by words, chroma by bytes); 34x34 is two pixels past a tile in both directions (the halo crosses a tile edge beside the image edge);
80x56 is ragged on both axes; 208x120 has several workgroups."""
import ctypes

import numpy as np
import pytest

import pixels_ref as px
import video_ref as vr

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = -1, -4
SIZES = [(16, 8), (18, 10), (20, 6), (34, 34), (80, 56), (208, 120)]
PHASES = (0, 1, 77)


def special_values(top):
    """Every k / top with its two f32 neighbours (top = 255, or 1023 for the 10-bit span), values below 0 and above 1, -0.0, the infinities and NaN."""
    k = np.arange(top + 1, dtype=F) / F(top)
    return np.concatenate([np.nextafter(k, F(-np.inf)), k, np.nextafter(k, F(np.inf)),
                           np.array([-0.0, -1e-45, -1e-3, -2.0, -3e38, 1.0 + 2.0 ** -23, 1.5, 300.0, 3e38, np.inf, -np.inf, np.nan, 1e-45, 0.5], F)]).astype(F)


_IMAGES = {}


def images(W, H, top=255):
    """The (W, H, 3) inputs of the kernel test at one size, as tests/test_gpu_pixels.py builds them: a slow ramp — 1/8 LSB per pixel along the columns, a
    third of an LSB between the channels, from below 0 to above `top` — with the special values at its odd flat indices, as many as fit; the small
    sizes take several images to hold them all.  Built once per (size, span) and never written to."""
    if (W, H, top) not in _IMAGES:
        n = W * H * 3
        sp = special_values(top)
        flat = np.arange(W * H, dtype=np.float64)[:, None]
        ramp = ((((flat / 8.0) % (top + 3.0)) - 1.0 + np.arange(3)[None, :] / 3.0) / top).astype(F).ravel()
        per = min(len(sp), n // 2)
        out = []
        for start in range(0, len(sp), per):
            chunk = sp[start:start + per]
            img = ramp.copy()
            img[1:2 * len(chunk):2] = chunk
            img = img.reshape(W, H, 3)
            img.flags.writeable = False
            out.append(img)
        _IMAGES[(W, H, top)] = out
    return _IMAGES[(W, H, top)]


def _top(format):
    return 1023 if vr.bits(format) == 10 else 255


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
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    diff = got != want
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:6].ravel().tolist(), got[diff][:6], want[diff][:6])


def _sums(W, H, seed=0):
    """Sums whose display covers black, saturated colours, mid greys and clipped white."""
    rng = np.random.default_rng(100 * W + H + seed)
    s = (np.exp2(rng.uniform(-9.0, 3.0, (W, H, 1))) * rng.uniform(0.3, 1.6, (W, H, 3))).astype(F)
    s[: W // 4, : H // 4] = 0.0
    return s


# ---------------------------------------------------------------- 1. the kernel, byte for byte
@pytest.mark.parametrize("size", SIZES)
def test_kernel_equals_the_restatement_in_every_layout(contexts, size):
    """All four formats x three sitings x two ranges, rounding."""
    W, H = size
    r = contexts(16, 8)                                       # de_debug_video is free of the context's size
    before = r.video()
    for format in vr.FORMATS:
        for n, img in enumerate(images(W, H, _top(format))[:3]):
            for siting in vr.SITINGS:
                for range_ in vr.RANGES:
                    got = r.debug_video(img, format=format, matrix="bt709", range=range_, siting=siting, mode="round")
                    _equal(got, vr.pack(img, format, "bt709", range_, siting, "round"), (size, n, format, siting, range_))
    assert r.video() == before                         # the debug entry point leaves the context's settings and counter alone


@pytest.mark.parametrize("size", SIZES)
def test_kernel_equals_the_restatement_in_every_mode_and_matrix(contexts, size):
    """Every mode and matrix, the dither at three phases, on a reduced grid: the layout, siting and range rotate with the case; every image of the size."""
    W, H = size
    r = contexts(16, 8)
    case = 0
    seen = {}
    for matrix in vr.MATRICES:
        for mode in vr.MODES:
            for phase in (PHASES if mode == "dither" else (0,)):
                format, siting, range_ = vr.FORMATS[case % 4], vr.SITINGS[(case // 2) % 3], vr.RANGES[case % 2]
                case += 1
                seed = 0 if phase == 0 else 0xC0FFEE + phase
                for n, img in enumerate(images(W, H, _top(format))):
                    got = r.debug_video(img, format=format, matrix=matrix, range=range_, siting=siting, mode=mode, seed=seed, phase=phase)
                    _equal(got, vr.pack(img, format, matrix, range_, siting, mode, seed, phase), (size, n, format, matrix, range_, siting, mode, phase))
                    if n == 0:
                        seen[(matrix, mode, phase)] = bytes(got)
    assert len(set(seen.values())) == len(seen) == 15         # no two cases gave the same frame


# ---------------------------------------------------------------- 2. end to end behind the display
def test_fetch_video_is_the_restatement_of_fetch_image(R, contexts):
    W, H = 80, 56
    r = contexts(W, H)
    sums = _sums(W, H)
    never = R.Renderer((W, H), (0, 1, 0), texture_source="constant")      # the feature is never touched on this one
    never.copy_textures()
    never.upload_hdr(sums, 3)
    r.upload_hdr(sums, 3)
    before = r.fetch_image()
    r.set_pixels(3, "round")
    before_px = r.fetch_pixels()
    assert (_bits(before) == _bits(never.fetch_image())).all()
    assert r.video() == dict(vr.DEFAULTS, last_phase=0, size=(W, H), frame_bytes=W * H * 3 // 2, plane_offsets=(0, W * H, W * H + 1), plane_strides=(W, W, W))
    for format in vr.FORMATS:
        for siting, matrix, range_, mode in (("left", "bt709", "limited", "round"), ("topleft", "bt2020", "full", "dither"), ("center", "bt601", "limited", "truncate")):
            r.set_video(format, matrix, range_, siting, mode, seed=5)
            want = vr.pack(before, format, matrix, range_, siting, mode, 5, 0)
            frame = r.fetch_video()
            _equal(frame, want, (format, siting))
            info = r.video()
            B = 2 if vr.bits(format) == 10 else 1
            assert info["frame_bytes"] == frame.nbytes == W * H * 3 // 2 * B and info["format"] == format and info["last_phase"] == 0
            view = r.fetch_video(copy=False)
            assert not view.flags.writeable
            _equal(np.array(view), want)
            del view
            planes = r.split_video(frame)
            y, cb, cr = vr.planes(frame, W, H, format)
            shift = 6 if format == "p010" else 0
            assert planes[0].shape == (H, W) and (planes[0] == y << shift).all() and planes[0].base is not None      # views, not copies
            if format in ("nv12", "p010"):
                assert len(planes) == 2 and planes[1].shape == (H // 2, W // 2, 2) and (planes[1][..., 0] == cb << shift).all() and (planes[1][..., 1] == cr << shift).all()
                assert info["plane_offsets"] == (0, W * H * B, W * H * B + B) and info["plane_strides"] == (W * B, W * B, W * B)
            else:
                assert len(planes) == 3 and (planes[1] == cb).all() and (planes[2] == cr).all()
                assert info["plane_offsets"] == (0, W * H * B, (W * H + W * H // 4) * B) and info["plane_strides"] == (W * B, W // 2 * B, W // 2 * B)
            # the other fetches give the same bytes between video fetches
            assert (_bits(r.fetch_image()) == _bits(before)).all() and (r.fetch_pixels() == before_px).all()
    assert r.render_to_video() not in (None, 0)
    # with bloom and auto-exposure on: whatever the display honours is inherited
    for x in (r, never):
        x.set_bloom(True, intensity=0.4)
        x.set_auto_exposure(True)
    shown = r.fetch_image()
    assert (_bits(shown) != _bits(before)).any()
    r.set_video("nv12", siting="left", mode="dither", seed=8)
    _equal(r.fetch_video(), vr.pack(shown, "nv12", mode="dither", seed=8))
    assert (_bits(r.fetch_image()) == _bits(shown)).all() and (_bits(never.fetch_image()) == _bits(shown)).all()
    for x in (r, never):
        x.set_bloom(False)
        x.set_auto_exposure(False)
    assert (_bits(r.fetch_image()) == _bits(before)).all() and (_bits(never.fetch_image()) == _bits(before)).all()
    assert (r.fetch_pixels() == before_px).all() and (_bits(r.fetch_hdr()) == _bits(never.fetch_hdr())).all()
    r.set_video()
    r.set_pixels()
    never.close()


def test_video_follows_output_scaling_and_the_hdr_signal(contexts):
    W, H = 80, 56
    r = contexts(W, H)
    r.upload_hdr(_sums(W, H, 3), 2)
    r.set_output_scale((48, 40), filter="mitchell")
    scaled = r.fetch_image()
    assert scaled.shape == (48, 40, 3)
    for format in ("i420", "p010"):
        r.set_video(format, siting="center")
        frame = r.fetch_video()
        _equal(frame, vr.pack(scaled, format, siting="center"), format)
        assert r.video()["size"] == (48, 40) and [p.shape for p in r.split_video(frame)][0] == (40, 48)
    assert (_bits(r.fetch_image()) == _bits(scaled)).all()
    r.set_output_scale(on=False)
    # PQ in a Rec.2020 container, NCL matrix, 10 bits, top-left siting: one setting away
    sdr = r.fetch_image()
    r.set_hdr_output(True, peak_nits=1000.0, gamut="rec2020", transfer="pq")
    signal = r.fetch_image()
    assert (_bits(signal) != _bits(sdr)).any()
    r.set_video("i010", matrix="bt2020", range="limited", siting="topleft")
    _equal(r.fetch_video(), vr.pack(signal, "i010", "bt2020", "limited", "topleft"))
    assert (_bits(r.fetch_image()) == _bits(signal)).all()
    r.set_hdr_output(False)
    assert (_bits(r.fetch_image()) == _bits(sdr)).all()
    r.set_video()


# ---------------------------------------------------------------- 3. the ring
def _display(r, sums):
    r.upload_hdr(sums, 2)
    return r.fetch_image()


def test_video_ring_is_in_order_and_independent_of_the_other_rings(contexts):
    from digital_earth_amd import _native
    W, H = 80, 56
    r = contexts(W, H)
    L, h = r._lib, r._h
    frames = [_sums(W, H, seed=k + 1) for k in range(12)]
    r.set_pixels(4, "round")
    r.set_video("i420", mode="round")
    shown = [_display(r, s) for s in frames]
    n = W * H * 3 // 2
    vp, fp, bp = ctypes.POINTER(ctypes.c_uint8)(), ctypes.POINTER(ctypes.c_float)(), ctypes.POINTER(ctypes.c_uint8)()
    assert L.de_fetch_videoframe_end(h, ctypes.byref(vp)) == ERR_STATE          # an _end without a _begin
    # four _begins, then four _ends: the frames in order
    for k in range(4):
        r.upload_hdr(frames[k], 2)
        assert L.de_fetch_videoframe_begin(h) == 0
    assert L.de_fetch_videoframe_begin(h) == ERR_STATE                          # the fifth
    for k in range(4):
        assert L.de_fetch_videoframe_end(h, ctypes.byref(vp)) == 0
        _equal(np.ctypeslib.as_array(vp, shape=(n,)).copy(), vr.pack(shown[k], "i420"), k)
    assert L.de_fetch_videoframe_end(h, ctypes.byref(vp)) == ERR_STATE
    # interleaved: frame k goes to ring k % 3 (float, pixel, video), four deep each
    begin = (L.de_fetch_image_begin, L.de_fetch_pixels_begin, L.de_fetch_videoframe_begin)
    for k, s in enumerate(frames):
        r.upload_hdr(s, 2)
        assert begin[k % 3](h) == 0
    assert [b(h) for b in begin] == [ERR_STATE] * 3
    s = _native.DeVideo()
    s.struct_bytes, s.format, s.mode = ctypes.sizeof(s), 3, 1
    assert L.de_set_video(h, ctypes.byref(s)) == ERR_STATE                 # while video fetches are in flight
    assert r.video()["format"] == "i420"
    o = _native.DeOutputScale()
    o.struct_bytes, o.enabled, o.width, o.height, o.filter = ctypes.sizeof(o), 1, 48, 40, 0
    assert L.de_set_output_scale(h, ctypes.byref(o)) == ERR_STATE
    order = (2, 1, 0, 5, 8, 3, 4, 11, 7, 6, 10, 9)                         # any order of the three rings: each hands out its own oldest
    handed = {0: 0, 1: 0, 2: 0}
    for k in order:
        ring = k % 3
        j = ring + 3 * handed[ring]                                        # the oldest frame of that ring not handed out yet
        handed[ring] += 1
        if ring == 0:
            assert L.de_fetch_image_end(h, ctypes.byref(fp)) == 0
            assert (_bits(np.ctypeslib.as_array(fp, shape=(W, H, 3))) == _bits(shown[j])).all(), j
        elif ring == 1:
            assert L.de_fetch_pixels_end(h, ctypes.byref(bp)) == 0
            assert (np.ctypeslib.as_array(bp, shape=(H, W, 4)) == px.pack(shown[j], 4, "round")).all(), j
        else:
            assert L.de_fetch_videoframe_end(h, ctypes.byref(vp)) == 0
            _equal(np.ctypeslib.as_array(vp, shape=(n,)).copy(), vr.pack(shown[j], "i420"), j)
    assert L.de_fetch_videoframe_end(h, ctypes.byref(vp)) == ERR_STATE and L.de_fetch_pixels_end(h, ctypes.byref(bp)) == ERR_STATE and L.de_fetch_image_end(h, ctypes.byref(fp)) == ERR_STATE
    assert L.de_set_video(h, ctypes.byref(s)) == 0 and r.video()["format"] == "i010"
    r.set_video()
    r.set_pixels()


@pytest.mark.parametrize("lag", (1, 3))
def test_lagged_fetches_and_the_animated_phase(contexts, lag):
    W, H = 80, 56
    r = contexts(W, H)
    frames = [_sums(W, H, seed=k + 20) for k in range(5)]
    shown = [_display(r, s) for s in frames]
    r.set_video("nv12", mode="dither", seed=21, animate=True)
    sync = []
    for k, s in enumerate(frames):
        r.upload_hdr(s, 2)
        sync.append(r.fetch_video())
        assert r.video()["last_phase"] == k                         # the phase counts conversions ...
        _equal(sync[k], vr.pack(shown[k], "nv12", mode="dither", seed=21, phase=k), k)      # ... and is part of the bytes
    r.set_video("nv12", mode="dither", seed=21, animate=True)       # resets the counter
    got = []
    for k, s in enumerate(frames):
        r.upload_hdr(s, 2)
        got.append(r.fetch_video(lag=lag))
    assert all(g is None for g in got[:lag])
    with pytest.raises(RuntimeError):
        r.fetch_video()                                              # lagged fetches are in flight
    assert r.fetch_pending() is None and r.fetch_pending(pixels=True) is None      # the other rings have nothing, and the video ring is left alone
    tail = r.fetch_pending(all_images=True, video=True)
    seq = got[lag:] + tail
    assert len(tail) == lag and len(seq) == len(frames) and r.fetch_pending(video=True) is None
    for k in range(len(frames)):
        _equal(seq[k], sync[k], k)
    r.set_video("nv12", mode="dither", seed=21, animate=False)      # animate = 0: the same frame gives the same bytes, phase 0
    a, b = r.fetch_video(), r.fetch_video()
    _equal(a, b)
    _equal(a, vr.pack(shown[-1], "nv12", mode="dither", seed=21, phase=0))
    assert r.video()["last_phase"] == 0
    r.set_video()


# ---------------------------------------------------------------- 4. errors, the viewer
def test_every_error_answers_its_code(contexts):
    from digital_earth_amd import _native
    W, H = 16, 8
    r = contexts(W, H)
    L, h = r._lib, r._h

    def settings(**kw):
        s = _native.DeVideo()
        s.struct_bytes, s.format, s.matrix, s.range, s.siting, s.mode, s.seed, s.animate = ctypes.sizeof(s), 0, 0, 0, 0, 1, 0, 0
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    r.set_video("i010", "bt601", "full", "center", "dither", seed=4, animate=True)
    held = r.video()
    for kw in (dict(struct_bytes=28), dict(struct_bytes=36), dict(format=-1), dict(format=4), dict(matrix=-1), dict(matrix=3), dict(range=-1), dict(range=2),
               dict(siting=-1), dict(siting=3), dict(mode=-1), dict(mode=3)):
        assert L.de_set_video(h, ctypes.byref(settings(**kw))) == ERR_INVALID, kw
        assert r.video() == held                       # a refused call changes nothing
    assert L.de_set_video(h, None) == ERR_INVALID and L.de_set_video(None, ctypes.byref(settings())) == ERR_INVALID
    assert L.de_get_video(h, None, None) == ERR_INVALID
    got = _native.DeVideo()
    assert L.de_get_video(h, ctypes.byref(got), None) == 0
    assert (got.struct_bytes, got.format, got.matrix, got.range, got.siting, got.mode, got.seed, got.animate) == (32, 3, 1, 1, 1, 2, 4, 1)
    r.upload_hdr(_sums(W, H), 1)
    out = np.empty(W * H * 3, np.uint8)
    assert L.de_fetch_video(h, out.ctypes.data, ctypes.c_uint64(out.nbytes - 1)) == ERR_INVALID      # a short out_bytes
    assert L.de_fetch_video(h, None, ctypes.c_uint64(out.nbytes)) == ERR_INVALID
    assert L.de_fetch_video(h, out.ctypes.data, ctypes.c_uint64(out.nbytes)) == 0
    assert L.de_fetch_videoframe_view(h, None) == ERR_INVALID and L.de_fetch_videoframe_end(h, None) == ERR_INVALID and L.de_render_to_video(None, None) == ERR_INVALID
    img = np.zeros((W, H, 3), F)
    for kw in (dict(struct_bytes=20), dict(format=4), dict(matrix=3), dict(range=2), dict(siting=3), dict(mode=3)):
        assert L.de_debug_video(h, img.ctypes.data, W, H, ctypes.byref(settings(**kw)), 0, out.ctypes.data) == ERR_INVALID, kw
    for w, hh in ((15, 8), (16, 7), (0, 8), (16, 0), (-2, 8)):      # an odd or empty size cannot be 4:2:0
        assert L.de_debug_video(h, img.ctypes.data, w, hh, ctypes.byref(settings()), 0, out.ctypes.data) == ERR_INVALID, (w, hh)
    assert L.de_debug_video(h, img.ctypes.data, 14, 6, ctypes.byref(settings()), 0, out.ctypes.data) == 0      # any even size
    # An odd output size answers DE_ERR_STATE from the video calls, but de_set_output_scale admits multiples of 16 x 8 only and refuses an odd size
    # itself (include/digital_earth_output_scale.h, unchanged): the state cannot be reached through the ABI, and the video calls go on at the size held.
    o = _native.DeOutputScale()
    o.struct_bytes, o.enabled, o.width, o.height, o.filter = ctypes.sizeof(o), 1, 15, 7, 0
    assert L.de_set_output_scale(h, ctypes.byref(o)) == ERR_INVALID
    assert r.output_size() == (W, H) and L.de_fetch_video(h, out.ctypes.data, ctypes.c_uint64(out.nbytes)) == 0
    for name, kw in (("format", dict(format="yuy2")), ("matrix", dict(matrix="smpte240")), ("range", dict(range="video")), ("siting", dict(siting="right")), ("mode", dict(mode="blue noise"))):
        with pytest.raises(ValueError):
            r.set_video(**kw)
    with pytest.raises(ValueError):
        r.fetch_video(lag=4)
    r.set_video()
    assert {k: v for k, v in r.video().items() if k in vr.DEFAULTS} == vr.DEFAULTS


def test_earth_viewer_hands_out_and_records_video_frames(tmp_path):
    from digital_earth_amd import y4m
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(64, 32), texture_source="synthetic", texture_size=(1024, 512), seed=5)
    a, b, c, d = EarthViewer(**kw), EarthViewer(**kw), EarthViewer(**kw), EarthViewer(**kw)
    for v in (b, c, d):
        v.renderer.set_video("i420", siting="left")
    floats = [a.frame(spp=1).copy() for k in range(3)]
    got = [b.frame(spp=1, video=True) for k in range(3)]
    for k in range(3):
        _equal(got[k], vr.pack(floats[k], "i420"), k)
    piped = [c.frame(spp=1, pipelined=1, video=True) for k in range(3)]
    assert piped[0] is None
    _equal(piped[1], got[0]); _equal(piped[2], got[1]); _equal(c.finish(video=True), got[2])
    assert c.finish(video=True) is None
    for bad in (dict(pixels=True), dict(hdr_pixels=True)):
        with pytest.raises(ValueError):
            b.frame(spp=1, video=True, **bad)
    path = str(tmp_path / "fly.y4m")
    assert d.record(path, 3, spp=1, fps=(25, 1)) == 3
    tokens, frames = y4m.read(path)
    assert tokens == ["YUV4MPEG2", "W64", "H32", "F25:1", "Ip", "A1:1", "C420mpeg2", "XCOLORRANGE=LIMITED"]
    assert len(frames) == 3
    for k in range(3):
        _equal(np.frombuffer(frames[k], np.uint8), got[k], k)
    d.renderer.set_video("nv12")
    with pytest.raises(ValueError):
        d.record(str(tmp_path / "no.y4m"), 1)
    for v in (a, b, c, d):
        v.close()
