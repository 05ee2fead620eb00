"""The panorama stage (include/digital_earth_panorama.h) and the rest of the chain on the GPU.  §25 says that a capture runs the chain as
it stands — denoiser, manual exposure, the SDR or HDR display transform, the look — and that every pack and every encoder behind the seam inherits the
360° frame; here each of those is held, exactly: the stage's output equals the numpy restatement (tests/panorama_ref.py, the device's own de_sincos and
square root handed in) of six faces obtained with the stage OFF through the same chain, and each downstream output equals its own reference on that
image.  The lagged rings deliver the synchronous bytes at the panorama's size, and every buffer sized from the output follows it larger and smaller.

One square context: N = 16 (de_create's smallest square), synthetic maps, 2 samples per face, one fixed oblique frame.  The six plain faces (SDR, no look,
apron 1) are rendered once and shared, never written to."""
import numpy as np
import pytest

import hdr_output_ref as ho
import jpeg_ref as jr
import panorama_ref as ref
import pixels_ref as px
import png_ref as pr
import video_ref as vr

pytestmark = pytest.mark.gpu

F = np.float32
ERR_STATE = -4
N = 16
SPP = 2
_f = np.array([2.0, -1.0, 2.0]) / 3.0
_u = np.array([1.0, 2.0, 0.0]) / np.sqrt(5.0)
_u = _u - _f * (_u @ _f)
_u /= np.linalg.norm(_u)
BASIS = np.stack([np.cross(_f, _u), _u, _f])        # rows r, u, f with r = f x u: an explicit frame, so that no capture depends on the camera's look
POS = (-5.5e6, 1.0e6, 5.5e6)                        # 1.23 planet radii from the centre: the disc spans 108°, several faces see it
EQUIRECT = dict(projection="equirect", aperture=180.0, apron=1, supersample=2)
TAUS = (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01)


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    r = R.Renderer((N, N), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512))
    r.copy_textures()
    yield r
    r.close()


def _camera(r, pos=POS):
    r.set_camera_pos(*pos)
    r.set_look_at(0.0, 0.0, 0.0)
    r.set_up(0.0, 1.0, 0.0)
    r.set_fov(0.4)
    r.set_aspect_scale(1.0)
    r.vignette_strength = 0.0                                       # captures refuse a vignette: it would print every face's border


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(got, want, what=""):
    """Exact: floats bit for bit, everything else value for value (bytes as bytes)."""
    if isinstance(want, (bytes, bytearray, memoryview)):
        assert bytes(got) == bytes(want), (what, len(bytes(got)), len(bytes(want)))
        return
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    a, b = (_bits(got), _bits(want)) if got.dtype == F else (got, want)
    diff = a != b
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def _differ(a, b):
    return bool((_bits(a) != _bits(b)).any())


def _face_camera(r, face):
    cam = r.panorama_face_camera(face)
    r.set_look_at(*cam["look_at"]); r._params.up[0], r._params.up[1], r._params.up[2] = cam["up"]; r._push_params()
    r.set_fov(cam["fov"]); r.set_aspect_scale(1.0)


def _faces_with_the_stage_off(r, size, frame=None, pos=POS, **settings):
    """The six faces beside a capture: the stage off (its settings kept: the face cameras are theirs), the same cameras, the same seeds, fetch_image().
    frame(r): what renders a face once its camera is set and the frame is reset; None: accumulate(SPP)."""
    _camera(r, pos)
    r.set_panorama(size, basis=BASIS, on=False, **settings)
    assert r.output_size() == (N, N)
    faces = np.empty((6, N, N, 3), F)
    for face in range(6):
        _face_camera(r, face)
        r.reset_framebuffer()
        if frame is None:
            r.accumulate(SPP)
        else:
            frame(r)
        faces[face] = r.fetch_image()
    _camera(r, pos)
    return faces


def _capture(r, size, pos=POS, **settings):
    """Stage on at `size`, six captures through render_panorama under the chain as it stands; the camera is the caller's again afterwards."""
    _camera(r, pos)
    r.set_panorama(size, basis=BASIS, **settings)
    r.render_panorama(SPP, basis=BASIS)
    assert r.panorama["captured"] == (0, 1, 2, 3, 4, 5) and r.output_size() == tuple(size)


def _restated(r, faces, size, projection="equirect", aperture=180.0, apron=1, supersample=2):
    sincos, sqrt = (lambda x: (r.debug_math(2, x), r.debug_math(3, x))), (lambda x: r.debug_math(8, x))
    return ref.panorama(faces, size, projection, aperture, apron, supersample, BASIS, sincos=sincos, sqrt=sqrt)


def _off(r):
    r.set_panorama((64, 32), basis=BASIS, on=False)
    _camera(r)


@pytest.fixture(scope="module")
def plain(ctx):
    """The six plain faces: SDR, no look, no denoiser, apron 1.  Rendered once, read-only."""
    faces = _faces_with_the_stage_off(ctx, (64, 32), **EQUIRECT)
    assert sum(len(np.unique(faces[k])) > 8 for k in range(6)) >= 2      # a picture on several faces (those that look away from the planet see black space)
    faces.flags.writeable = False
    return faces


# ---------------------------------------------------------------- 1. the look
def _cube3(seed):
    from digital_earth_amd import cube as cube_mod
    return cube_mod.Cube("3d", 3, np.random.default_rng(seed).uniform(0.0, 1.0, 27 * 3).astype(F))


def test_a_capture_under_a_look_holds_graded_faces(ctx, plain):
    r = ctx
    size = (64, 32)
    first, second = dict(cube=_cube3(3), strength=0.37), dict(cube=_cube3(4), strength=1.0)
    try:
        r.set_look(**first)
        _capture(r, size, **EQUIRECT)
        shown = r.fetch_image()
        # the slots hold graded pixels: another look, or none, changes nothing until faces are captured again
        r.set_look(**second)
        _same(r.fetch_image(), shown, "another look after the capture")
        r.set_look(enabled=False)
        _same(r.fetch_image(), shown, "no look after the capture")
        r.set_look(**second)
        r.render_panorama(SPP, basis=BASIS)
        again = r.fetch_image()
        assert _differ(again, shown)
        for kw, got in ((first, shown), (second, again)):
            r.set_look(**kw)
            graded = _faces_with_the_stage_off(r, size, **EQUIRECT)
            assert _differ(graded, plain)                           # the look did grade the faces
            _same(got, _restated(r, graded, size), ("the panorama of six graded faces", kw["strength"]))
    finally:
        r.set_look(enabled=False)
        _off(r)


# ---------------------------------------------------------------- 2. the HDR display output
def test_a_capture_under_the_hdr_transform_and_its_packed_pixels(ctx, plain):
    r = ctx
    size = (64, 32)
    r.set_pixels(3, "round")
    _capture(r, size, **EQUIRECT)
    sdr = r.fetch_image(), r.fetch_pixels()
    _same(sdr[0], _restated(r, plain, size), "SDR")
    try:
        for transfer in ("pq", "hlg"):
            config = dict(peak_nits=1000.0, gamut="rec709", transfer=transfer)
            r.set_hdr_output(True, pixel_format="rgb10a2", mode="round", **config)
            _capture(r, size, **EQUIRECT)
            shown = r.fetch_image()
            assert _differ(shown, sdr[0])
            got10 = r.fetch_hdr_pixels()
            assert got10.shape == (size[1], size[0]) and got10.dtype == np.uint32
            _same(got10, ho.pack(shown, "rgb10a2", "round"), (transfer, "rgb10a2"))
            r.set_hdr_output(True, pixel_format="rgb16", mode="dither", seed=5, **config)      # the pack alone changes: the slots stay
            got16 = r.fetch_hdr_pixels()
            assert got16.shape == (size[1], size[0], 3) and got16.dtype == np.uint16
            _same(got16, ho.pack(shown, "rgb16", "dither", seed=5), (transfer, "rgb16"))
            _same(r.fetch_image(), shown, transfer)
            signal = _faces_with_the_stage_off(r, size, **EQUIRECT)
            assert _differ(signal, plain)
            _same(shown, _restated(r, signal, size), ("the panorama of six HDR-signal faces", transfer))
        r.set_hdr_output(False)
        _capture(r, size, **EQUIRECT)
        _same(r.fetch_image(), sdr[0], "off again")
        _same(r.fetch_pixels(), sdr[1], "off again, the SDR bytes")
    finally:
        r.set_hdr_output(False)
        r.set_pixels()
        _off(r)


# ---------------------------------------------------------------- 3. video frames
@pytest.mark.parametrize("size", [(64, 32), (48, 24)])
def test_video_frames_of_the_panorama(ctx, plain, size):
    """48 x 24: chroma planes of 24 x 12, a partial tile of the pack on both axes."""
    r = ctx
    try:
        _capture(r, size, **EQUIRECT)
        shown = r.fetch_image()
        _same(shown, _restated(r, plain, size), size)
        for kw in (dict(format="nv12"), dict(format="i420", siting="center"), dict(format="p010", matrix="bt2020", siting="topleft", mode="dither", seed=3)):
            r.set_video(**kw)
            got = r.fetch_video()
            assert got.nbytes == size[0] * size[1] * 3 // 2 * (2 if kw["format"] == "p010" else 1) and r.video()["size"] == size
            _same(got, vr.pack(shown, **kw), (size, kw["format"]))
            view = r.fetch_video(copy=False)
            _same(np.array(view), got, (size, kw["format"], "view"))
            del view
    finally:
        r.set_video()
        _off(r)


# ---------------------------------------------------------------- 4. denoised faces
def test_a_capture_with_the_denoiser_on(ctx, plain):
    r = ctx
    size = (64, 32)
    try:
        r.set_denoise(True)
        _capture(r, size, **EQUIRECT)
        shown = r.fetch_image()
        denoised = _faces_with_the_stage_off(r, size, **EQUIRECT)
        assert _differ(denoised, plain)
        _same(shown, _restated(r, denoised, size), "the panorama of six denoised faces")
    finally:
        r.set_denoise(False)
        _off(r)


# ---------------------------------------------------------------- 5. adaptive faces
def _adaptive(tau):
    return lambda r: r.render_adaptive(tau, 32, min_spp=16, round_spp=16)


def test_a_capture_of_adaptive_frames(ctx):
    """Faces whose tiles stopped at different counts: the display divides every tile by its own count, and the capture takes that image."""
    r = ctx
    size = (64, 32)
    try:
        # the first threshold that leaves both counts on some face, found with the stage off
        for tau in TAUS:
            counts = []

            def frame(r, tau=tau):
                _adaptive(tau)(r)
                counts.append(r.tile_spp().copy())
            faces = _faces_with_the_stage_off(r, size, frame=frame, **EQUIRECT)
            if any(set(np.unique(c).tolist()) == {16, 32} for c in counts):
                break
        else:
            pytest.fail("no threshold of %s leaves mixed tile counts on a face" % (TAUS,))
        assert all(c.shape == (N // 8, N // 8) and set(np.unique(c).tolist()) <= {16, 32} for c in counts)
        print("adaptive faces: threshold %g, tile counts %s" % (tau, [c.ravel().tolist() for c in counts]))
        _camera(r)
        r.set_panorama(size, basis=BASIS, **EQUIRECT)
        for face in range(6):
            _face_camera(r, face)
            r.reset_framebuffer()
            _adaptive(tau)(r)
            assert (r.tile_spp() == counts[face]).all(), face       # the same adaptive frame as beside it
            r.capture_panorama_face(face)
        _same(r.fetch_image(), _restated(r, faces, size), "the panorama of six adaptive faces")
    finally:
        r.reset_framebuffer()
        _off(r)


# ---------------------------------------------------------------- 6. the fisheye end to end
@pytest.mark.parametrize("case", [((32, 32), 180.0), ((48, 48), 220.0)])
def test_fisheye_end_to_end(ctx, plain, case):
    r = ctx
    size, aperture = case
    settings = dict(projection="fisheye", aperture=aperture, apron=1, supersample=2)
    try:
        r.set_pixels(3, "round")
        r.set_png()
        _capture(r, size, **settings)
        p = r.panorama
        assert p["projection"] == "fisheye" and p["aperture"] == aperture and p["size"] == size
        shown = r.fetch_image()
        _same(shown, _restated(r, plain, size, **settings), case)
        assert (shown[0, 0] == 0).all() and len(np.unique(shown)) > 64      # the corner lies beyond the circle; a picture inside it
        pixels = r.fetch_pixels()
        _same(pixels, px.pack(shown, 3, "round"), case)
        png = r.fetch_png()
        _same(png, pr.encode(pixels), case)
        _same(pr.decode(png)[0], pixels, case)
    finally:
        r.set_pixels()
        _off(r)


# ---------------------------------------------------------------- 7. lagged rings at the panorama's size
def _set_outputs(r):
    r.set_pixels(3, "round")
    r.set_video("i420")
    r.set_jpeg(80)
    r.set_png()


def _reset_outputs(r):
    r.set_pixels(); r.set_video(); r.set_jpeg()


@pytest.mark.parametrize("lag", (1, 2, 3))
def test_lagged_fetches_give_the_synchronous_bytes_at_the_panoramas_size(R, ctx, lag):
    """Five panoramas from five camera positions, the frame fixed (a changed basis is a de_set_panorama, which lagged fetches refuse): every ring at
    once, each delivering the synchronous loop's frames in order."""
    r = ctx
    size = (48, 24)
    fetches = ("fetch_image", "fetch_pixels", "fetch_video", "fetch_jpeg", "fetch_png")
    positions = [(POS[0] + 2.0e5 * k, POS[1] - 1.0e5 * k, POS[2]) for k in range(5)]
    try:
        _set_outputs(r)
        _camera(r)
        r.set_panorama(size, basis=BASIS, **EQUIRECT)

        def frame(pos):
            r.set_camera_pos(*pos)
            r.render_panorama(SPP, basis=BASIS)

        sync = {f: [] for f in fetches}
        for pos in positions:
            frame(pos)
            for f in fetches:
                got = getattr(r, f)()
                sync[f].append(got if isinstance(got, bytes) else np.array(got))
        assert sync["fetch_image"][0].shape == size + (3,) and sync["fetch_pixels"][0].shape == (size[1], size[0], 3)
        assert sync["fetch_video"][0].nbytes == size[0] * size[1] * 3 // 2
        for f in fetches:
            raw = [g if isinstance(g, bytes) else g.tobytes() for g in sync[f]]
            assert len(set(raw)) == len(raw), f                     # no two frames alike: an order could show
        lagged = {f: [] for f in fetches}
        for pos in positions:
            frame(pos)
            for f in fetches:
                lagged[f].append(getattr(r, f)(lag=lag))
        assert all(g is None for f in fetches for g in lagged[f][:lag])
        with pytest.raises(R.DigitalEarthError) as e:
            r.set_panorama((64, 32), basis=BASIS, **EQUIRECT)       # refused while fetches are in flight
        assert e.value.code == ERR_STATE and r.output_size() == size and r.panorama["captured"] == (0, 1, 2, 3, 4, 5)
        tails = {"fetch_image": r.fetch_pending(all_images=True), "fetch_pixels": r.fetch_pending(all_images=True, pixels=True),
                 "fetch_video": r.fetch_pending(all_images=True, video=True), "fetch_jpeg": r.fetch_pending_jpeg(all_images=True),
                 "fetch_png": r.fetch_pending_png(all_images=True)}
        for f in fetches:
            seq = lagged[f][lag:] + tails[f]
            assert len(tails[f]) == lag and len(seq) == len(positions), f
            for k in range(len(positions)):
                _same(seq[k], sync[f][k], (f, lag, k))
    finally:
        r.fetch_pending(); r.fetch_pending(pixels=True); r.fetch_pending(video=True); r.fetch_pending_jpeg(); r.fetch_pending_png()
        _reset_outputs(r)
        _off(r)


# ---------------------------------------------------------------- 8. resizing
def test_every_output_follows_the_panoramas_size_larger_and_smaller(ctx, plain):
    """Pixels, video, JPEG and PNG set; the stage at 64 x 32, then 96 x 40, then 48 x 24, then off: every device buffer, staging buffer and ring cell
    sized from the output's width and height grows, then serves a frame below its capacity."""
    r = ctx
    video = dict(format="i010", siting="center")

    def outputs():
        return (r.fetch_image(), r.fetch_pixels(), r.fetch_video(), bytes(r.fetch_jpeg()), bytes(r.fetch_png()))

    try:
        _set_outputs(r)
        r.set_video(**video)
        _off(r)
        r.reset_framebuffer()
        r.accumulate(SPP)
        before = outputs()
        assert before[0].shape == (N, N, 3) and before[1].shape == (N, N, 3) and before[2].nbytes == N * N * 3
        for size in ((64, 32), (96, 40), (48, 24)):
            _capture(r, size, **EQUIRECT)
            shown, pixels, frame, jpeg, png = outputs()
            _same(shown, _restated(r, plain, size), size)
            _same(pixels, px.pack(shown, 3, "round"), size)
            _same(frame, vr.pack(shown, **video), size)
            _same(jpeg, bytes(jr.encode(shown, 80, None)), size)
            _same(png, bytes(pr.encode(pixels)), size)
            assert r.jpeg()["size"] == size and r.png()["size"] == size and r.video()["size"] == size
            # the views (the staging buffers) and the rings (every cell) at this size
            for fetch, want in ((r.fetch_image, shown), (r.fetch_pixels, pixels), (r.fetch_video, frame)):
                view = fetch(copy=False)
                _same(np.array(view), want, (size, "view"))
                del view
            for fetch, pending, want in ((r.fetch_image, {}, shown), (r.fetch_pixels, dict(pixels=True), pixels), (r.fetch_video, dict(video=True), frame)):
                got = [fetch(lag=2) for k in range(5)] + r.fetch_pending(all_images=True, **pending)
                assert [g is None for g in got] == [True, True] + [False] * 5
                for g in got[2:]:
                    _same(g, want, (size, "ring"))
            for fetch, pending, want in ((r.fetch_jpeg, r.fetch_pending_jpeg, jpeg), (r.fetch_png, r.fetch_pending_png, png)):
                got = [fetch(lag=1) for k in range(3)] + pending(all_images=True)
                assert got[0] is None and len(got) == 4
                for g in got[1:]:
                    _same(g, want, (size, "coded ring"))
        _off(r)
        assert r.output_size() == (N, N)
        r.reset_framebuffer()
        r.accumulate(SPP)
        after = outputs()
        for k in range(5):
            _same(after[k], before[k], ("off again", k))
    finally:
        _reset_outputs(r)
        _off(r)
