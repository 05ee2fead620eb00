"""The scene-linear panorama (include/digital_earth_environment.h) on the GPU, bit-exact against restatements the project already has:
a linear face is fetch_hdr() / float32(spp) of its render (per tile inside an adaptive frame; fetch_denoised_hdr() with the denoised source); the
row-major resampling equals tests/panorama_ref.py's image with the device's own de_sincos and square root handed to it; the file is tests/exr_ref.py's
encoding of that image oriented as the EXR output orients a frame; digital_earth_amd.exr.read gives the samples back.

Shapes, the smallest at which each thing can go wrong.  Capture: N = 16 is one partial 32 x 32 tile, N = 48 is 2 x 2 tiles with the last partial (a
swapped tile index leaves a quadrant wrong), N = 64 for the adaptive frame (8 x 8 count tiles, whole capture tiles).  Resampling: panorama_ref.MULTI_TILE
(3 x 2, 2 x 3, 2 x 2, 3 x 3 tiles, the last partial) over panorama_ref.FACE_SIZES and the 32 x 32 fisheye at 360°, S = 1, 3, 4."""
import ctypes

import numpy as np
import pytest

import exr_ref as xr
import panorama_ref as ref
import pixels_ref as px
from digital_earth_amd import exr

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = -1, -4
N = 16
SCENE = dict(texture_source="synthetic", texture_size=(1024, 512))
_f = np.array([2.0, -1.0, 2.0]) / 3.0
_u = np.array([1.0, 2.0, 0.0]) / np.sqrt(5.0)
_u = _u - _f * (_u @ _f)
_u /= np.linalg.norm(_u)
OBLIQUE = np.stack([np.cross(_f, _u), _u, _f])      # rows r, u, f with r = f x u, as the renderer's right, up, forward
POSITIONS = ((-5.5e6, 1.0e6, 5.5e6), (5.0e6, 2.0e6, 5.5e6), (-2.0e6, 7.0e6, 3.0e6), (6.5e6, -1.0e6, -4.0e6))


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    """One square Renderer of N = 16 on small synthetic maps, shared by every test; a test leaves the panorama off and the EXR settings at their defaults."""
    r = R.Renderer((N, N), (0, 1, 0), **SCENE)
    r.copy_textures()
    yield r
    r.close()


def device_leaves(r):
    """The device's de_sincos (de_debug_math 2 and 3 are its two outputs) and its square root (8), for the restatement."""
    return (lambda x: (r.debug_math(2, x), r.debug_math(3, x))), (lambda x: r.debug_math(8, x))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def _same_bytes(got, want, what=""):
    got, want = bytes(got), bytes(want)
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("%s: %d bytes against %d, first difference at %d" % (what, len(got), len(want), first))


def _oriented(field):
    """A (W, H, 3) field of the library -> (H, W, 3) rows top-down, as the EXR output orients a frame: file[r][x] = field[x][H - 1 - r]."""
    return np.ascontiguousarray(np.asarray(field)[:, ::-1].transpose(1, 0, 2))


def _field(rows):
    """The inverse: an (H, W, 3) image as exr.read returns it -> the library's (W, H, 3) field."""
    return np.ascontiguousarray(np.asarray(rows)[::-1].transpose(1, 0, 2))


def _camera(r, pos=POSITIONS[0]):
    r.set_camera_pos(*pos)
    r.set_look_at(0.0, 0.0, 0.0)
    r.set_up(0.0, 1.0, 0.0)
    r.set_fov(0.4)
    r.set_aspect_scale(1.0)
    r.vignette_strength = 0.0


def _off(r):
    r.set_panorama((64, 32), on=False)
    r.set_exr()


def linear_faces(n, seed):
    """Scene-linear content: values up to 1e4, one in eight negative."""
    rng = np.random.default_rng(2600 + seed)
    v = rng.random((6, n, n, 3), dtype=F) * F(1e4)
    return np.where(rng.random((6, n, n, 3)) < 0.125, -v, v).astype(F)


def _image_of(r, faces, size, projection, aperture, apron, S, basis):
    """The (W, H, 3) image inside a FLOAT file without compression: the file's samples are the image's bits."""
    data = r.debug_environment_exr(faces, size, projection, aperture, apron, S, basis, pixel_type="float", compression="none")
    back, info = exr.read(data)
    assert back.dtype == F and (info["width"], info["height"]) == tuple(size) and info["pixel_type"] == "float" and info["compression"] == "none"
    return _field(back), data


# ---------------------------------------------------------------- 1. the capture kernel
@pytest.mark.parametrize("n", (16, 48))
def test_linear_face_is_fetch_hdr_over_spp(R, n):
    r = R.Renderer((n, n), (0, 1, 0), seed=3, **SCENE)
    r.copy_textures()
    _camera(r)
    assert r.environment == dict(captured=())
    r.set_panorama((64, 32), apron=1, supersample=1, basis=r.camera_basis())
    for face in range(6):
        cam = r.panorama_face_camera(face)
        r.set_look_at(*cam["look_at"]); r._params.up[0], r._params.up[1], r._params.up[2] = cam["up"]; r._push_params()
        r.set_fov(cam["fov"])
        r.reset_framebuffer()
        spp = 1 + face % 2
        r.accumulate(spp)
        r.capture_environment_face(face)
        want = (r.fetch_hdr() / F(spp)).astype(F)
        got = r.fetch_environment_face(face)
        _same(got, want, (n, face))
        assert r.environment["captured"] == tuple(range(face + 1)) and r.panorama["captured"] == ()
    seen = [r.fetch_environment_face(k) for k in range(6)]
    assert sum(len(np.unique(s)) > n for s in seen) >= 3 and max(float(s.max()) for s in seen) > 0.0      # pictures of the planet, not flat fields
    assert any(np.abs(s - s.transpose(1, 0, 2)).max() > 0 for s in seen)                                  # so that a missing transposition shows
    r.reset_framebuffer()                                           # de_reset keeps the slots
    assert r.environment["captured"] == (0, 1, 2, 3, 4, 5)
    r.close()


def test_linear_face_of_an_adaptive_frame_is_divided_tile_by_tile(R):
    n = 64                                                          # 8 x 8 count tiles over 2 x 2 capture tiles
    r = R.Renderer((n, n), (0, 1, 0), texture_source="synthetic", texture_size=(2048, 1024), seed=11)
    r.set_fov(0.42)
    r.copy_textures()
    for tau in (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01):      # the first threshold that leaves tiles at different counts (tests/test_gpu_exr.py)
        r.reset_framebuffer()
        while r.accumulate_adaptive(tau, 32, min_spp=4, round_spp=4) > 0:
            pass
        counts = np.asarray(r.tile_spp())
        if len(np.unique(counts)) > 1:
            break
    assert counts.shape == (n // 8, n // 8) and counts.min() >= 4 and len(np.unique(counts)) > 1      # a mixed-count frame
    per_pixel = np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1).astype(F)[..., None]
    r.vignette_strength = 0.0
    r.set_panorama((64, 32))
    r.capture_environment_face(2)                                   # the library does not check the camera of a capture
    _same(r.fetch_environment_face(2), (r.fetch_hdr() / per_pixel).astype(F), "adaptive")
    assert r.environment["captured"] == (2,)
    r.close()


def test_linear_face_of_the_denoised_source_is_fetch_denoised_hdr(R, ctx):
    r = ctx
    _camera(r)
    r.set_panorama((64, 32))
    r.set_exr(source="denoised")
    try:
        with pytest.raises(R.DigitalEarthError) as mine:
            r.capture_environment_face(0)                           # the denoiser is off: de_fetch_denoised_hdr's refusal
        with pytest.raises(R.DigitalEarthError) as theirs:
            r.fetch_denoised_hdr()
        assert mine.value.code == theirs.value.code == ERR_STATE and str(mine.value) == str(theirs.value) and r.environment["captured"] == ()
        r.set_denoise(True)
        r.reset_framebuffer()
        r.accumulate(2)
        r.capture_environment_face(0)
        _same(r.fetch_environment_face(0), np.ascontiguousarray(r.fetch_denoised_hdr()).astype(F), "denoised")
    finally:
        r.set_denoise(False)
        _off(r)


# ---------------------------------------------------------------- 2. the row-major resampling kernel
@pytest.mark.parametrize("output", ref.MULTI_TILE + [((32, 32), "fisheye", 360.0)])
def test_resampling_equals_the_restatement_bit_for_bit(ctx, output):
    size, projection, aperture = output
    sincos, sqrt = device_leaves(ctx)
    held, held_env, held_exr = ctx.panorama, ctx.environment, ctx.exr()
    for n, apron in ref.FACE_SIZES:
        for S in (1, 3, 4):
            basis = OBLIQUE if S == 3 else None
            faces = linear_faces(n, seed=S + 10 * apron + n)
            got, _ = _image_of(ctx, faces, size, projection, aperture, apron, S, basis)
            want = ref.panorama(faces, size, projection, aperture, apron, S, basis, sincos=sincos, sqrt=sqrt)
            _same(got, want, (output, n, apron, S))
            assert got.min() < 0.0 and got.max() > 1000.0 and len(np.unique(got)) > got.size // 8      # scene-linear content, not a flat field
    now = ctx.panorama
    assert now["on"] == held["on"] and now["size"] == held["size"] and ctx.environment == held_env and ctx.exr() == held_exr      # the debug entry point leaves the context alone


@pytest.mark.parametrize("S", (1, 4))
@pytest.mark.parametrize("output", ref.MULTI_TILE + [((32, 32), "fisheye", 360.0)])
def test_linear_field_comes_out_as_the_float64_direction_field(ctx, output, S):
    """tests/test_gpu_panorama.py's comparison with something not written from the header, through the row-major kernel and the file: within
    panorama_ref.LINEAR_BOUND, the project's own measured bound, and exactly 0 beyond the fisheye's circle."""
    size, projection, aperture = output
    worst = 0.0
    for apron in (1, 4):
        for basis in (None, OBLIQUE):
            got, _ = _image_of(ctx, ref.f64_linear_faces(N, apron, basis), size, projection, aperture, apron, S, basis)
            want, inside, outside = ref.f64_linear_image(size, projection, aperture, basis, S)
            assert got.shape == want.shape and inside.sum() > inside.size // 2
            assert (got[outside] == 0).all(), (output, S, apron)
            err = float(np.abs(got.astype(np.float64) - want)[~outside].max())
            print("linear field through the row-major kernel %s S %d apron %d %s: max error %.3e" % (output, S, apron, "oblique" if basis is not None else "axes", err))
            worst = max(worst, err)
    assert 0.0 < worst <= ref.LINEAR_BOUND[S], (worst, ref.LINEAR_BOUND[S])


def test_constant_faces_come_out_constant(ctx):
    for size, projection, aperture in (((64, 32), "equirect", 180.0), ((48, 72), "equirect", 180.0), ((32, 32), "fisheye", 360.0)):
        for S in (1, 2, 3, 4):
            for value in (0.0, 0.3, 70000.0):
                faces = np.full((6, N, N, 3), value, F)
                got, _ = _image_of(ctx, faces, size, projection, aperture, 1, S, OBLIQUE)
                half, info = exr.read(ctx.debug_environment_exr(faces, size, projection, aperture, 1, S, OBLIQUE, pixel_type="half", compression="none"))
                assert half.dtype == np.float16 and half.shape == (size[1], size[0], 3)
                if projection == "equirect":
                    assert np.unique(_bits(got)).tolist() == [int(F(value).view(np.uint32))], (size, S, value)
                    assert np.unique(_bits(half)).tolist() == [int(np.float16(min(value, 65504.0)).view(np.uint16))], (size, S, value)
                    if value == 70000.0:
                        assert np.unique(_bits(half)).tolist() == [0x7BFF]
                else:
                    assert got.min() >= 0.0 and got.max() == F(value) and got[16, 16, 0] == F(value) and got[0, 0, 0] == 0.0
                    if value == 70000.0:
                        assert int(_bits(half).max()) == 0x7BFF and _bits(_field(half))[16, 16, 0] == 0x7BFF


# ---------------------------------------------------------------- 3. end to end
CASES = [((64, 32), "equirect", 180.0, dict(pixel_type="half", compression="zip")),
         ((96, 40), "equirect", 180.0, dict(pixel_type="float", compression="zips", scale=0.25, chunk_bytes=2048)),
         ((48, 48), "fisheye", 220.0, dict(pixel_type="half", compression="none"))]


def _restated_file(r, size, projection, aperture, supersample, settings):
    sincos, sqrt = device_leaves(r)
    faces = np.stack([r.fetch_environment_face(k) for k in range(6)])
    image = ref.panorama(faces, size, projection, aperture, 1, supersample, r.panorama["basis"], sincos=sincos, sqrt=sqrt)
    kw = dict(settings)
    return xr.encode(_oriented(image), kw.pop("pixel_type"), kw.pop("compression"), kw.pop("chunk_bytes", xr.DEFAULT_CHUNK), kw.pop("scale", 1.0)), image, faces


@pytest.mark.parametrize("case", CASES)
def test_end_to_end_file_equals_the_restatement_byte_for_byte(R, ctx, case):
    size, projection, aperture, settings = case
    r = ctx
    _camera(r)
    r.set_panorama(size, projection, aperture, apron=1, supersample=2)
    r.set_exr(**settings)
    try:
        with pytest.raises(R.DigitalEarthError) as e:
            r.fetch_exr()                                           # no linear face yet: as before this output existed
        assert e.value.code == ERR_STATE
        r.render_environment(1)
        assert r.environment["captured"] == (0, 1, 2, 3, 4, 5) and r.panorama["captured"] == () and r.current_spp == 0
        assert np.abs(r.panorama["basis"].astype(np.float64) - r.camera_basis()).max() < 1e-6      # the caller's camera is back
        got = r.fetch_exr()
        want, image, faces = _restated_file(r, size, projection, aperture, 2, settings)
        assert len(np.unique(image)) > 64 and image.max() > 0.0
        _same_bytes(got, want, case)
        back, info = exr.read(got)
        assert (info["width"], info["height"]) == size and back.shape == (size[1], size[0], 3) and info["pixel_type"] == settings["pixel_type"]
        _same(back, xr.convert(_oriented(image), settings.get("scale", 1.0), settings["pixel_type"]), "the samples")
        state = r.exr()
        assert state["size"] == size and state["capacity"] == xr.capacity(size[0], size[1], settings["pixel_type"], settings["compression"]) >= len(got)
        view = r.fetch_exr(copy=False)
        _same_bytes(view, got, "the view")
        del view
        p, n = r.render_to_exr()
        assert p and n and p - n == 16
        with pytest.raises(R.DigitalEarthError) as e:
            r.fetch_image()                                         # no display face: the shown panorama does not exist
        assert e.value.code == ERR_STATE
    finally:
        _off(r)


# ---------------------------------------------------------------- 4. the ring and the other fetches
@pytest.mark.parametrize("lag", (1, 2, 3))
def test_ring_delivers_the_synchronous_files_in_order(R, ctx, lag):
    r = ctx
    r.set_panorama((64, 32), supersample=1, basis=np.eye(3))
    r.set_exr(pixel_type="half", compression="zip", chunk_bytes=2048)
    try:
        def environment(pos):
            _camera(r, pos)
            r.render_environment(1, basis=np.eye(3))                # the frame fixed: a changed basis is a de_set_panorama, which a lagged fetch refuses
        sync = []
        for pos in POSITIONS:
            environment(pos)
            sync.append(r.fetch_exr())
        assert len({bytes(s) for s in sync}) == len(POSITIONS)
        got = []
        for k, pos in enumerate(POSITIONS):
            environment(pos)
            out = r.fetch_exr(lag=lag)
            assert (out is None) == (k < lag)
            if out is not None:
                got.append(out)
        got += r.fetch_pending_exr(all_images=True)
        assert len(got) == len(POSITIONS)
        for k in range(len(POSITIONS)):
            _same_bytes(got[k], sync[k], "lag %d environment %d" % (lag, k))
        assert r.fetch_pending_exr() is None
    finally:
        _off(r)


def test_display_and_linear_captures_of_one_render(R, ctx):
    import png_ref as pr
    r = ctx
    size = (64, 32)
    _camera(r)
    basis = r.camera_basis()
    r.set_pixels(3, "round")
    r.set_png()
    r.set_panorama(size, supersample=2, basis=basis)
    r.set_exr(pixel_type="float")
    try:
        r.render_panorama(1, basis=basis)                           # the display side alone
        alone = (r.fetch_image().copy(), bytes(r.fetch_png()))
        r.render_environment(1, basis=basis, display=True)
        assert r.environment["captured"] == r.panorama["captured"] == (0, 1, 2, 3, 4, 5)
        shown, png, file = r.fetch_image().copy(), bytes(r.fetch_png()), r.fetch_exr()
        _same(shown, alone[0], "fetch_image with and without the linear captures")
        assert png == alone[1]
        want, image, faces = _restated_file(r, size, "equirect", 180.0, 2, dict(pixel_type="float", compression="zip"))
        _same_bytes(file, want, "fetch_exr beside the display captures")
        assert png == bytes(pr.encode(px.pack(shown, 3, "round", 0, 0)))
        assert shown.min() >= 0.0 and shown.max() <= 1.0 and not np.array_equal(shown, image)      # display-referred beside scene-linear
        # fetch_image's own reference: the six faces with the stage off, the same cameras and seeds
        r.set_panorama(size, supersample=2, basis=basis, on=False)
        display_faces = np.empty((6, N, N, 3), F)
        for face in range(6):
            cam = r.panorama_face_camera(face)
            r.set_look_at(*cam["look_at"]); r._params.up[0], r._params.up[1], r._params.up[2] = cam["up"]; r._push_params()
            r.set_fov(cam["fov"])
            r.reset_framebuffer()
            r.accumulate(1)
            display_faces[face] = r.fetch_image()
            _same((r.fetch_hdr() / F(1)).astype(F), faces[face], "linear face %d against the same render with the stage off" % face)
        sincos, sqrt = device_leaves(r)
        _same(shown, ref.panorama(display_faces, size, "equirect", 180.0, 1, 2, basis, sincos=sincos, sqrt=sqrt), "fetch_image")
    finally:
        r.set_pixels(); _off(r)


# ---------------------------------------------------------------- 5. refusals
def _state(r):
    """Both masks and every setting a refused call could have touched (de_get_exr itself: Renderer.exr() also asks for the capacity, which a size
    beyond the limit refuses)."""
    from digital_earth_amd import _native
    p, s = r.panorama, _native.DeExr()
    assert r._lib.de_get_exr(r._h, ctypes.byref(s)) == 0
    return (p["on"], p["size"], p["projection"], p["supersample"], p["captured"], r.environment["captured"],
            (s.source, s.pixel_type, s.compression, s.chunk_bytes, s.scale), r.exr_aovs())


def test_refusals_leave_masks_and_settings_unchanged(R, ctx):
    r = ctx
    L, h = r._lib, r._h
    _camera(r)
    r.reset_framebuffer()
    r.accumulate(1)
    pinhole = r.fetch_exr()                                         # the stage off: the frame's own file
    # capture with the stage off
    before = _state(r)
    assert L.de_environment_capture(h, 0) == ERR_STATE and _state(r) == before
    out = np.full((N, N, 3), 7.0, F)
    assert L.de_fetch_environment_face(h, 0, out.ctypes.data) == ERR_STATE and (out == 7.0).all()      # not held
    r.set_panorama((64, 32))
    try:
        # sources that would print another face's camera or the face's border into the environment
        for source, switch in (("history", r.set_history), ("bloom", r.set_bloom), ("local_exposure", r.set_local_exposure)):
            r.set_exr(source=source)
            for on in (False, True):
                switch(on)
                before = _state(r)
                assert L.de_environment_capture(h, 0) == ERR_STATE and _state(r) == before, (source, on)
                assert ("camera" if source == "history" else "border") in L.de_last_error().decode()
            switch(False)
        r.set_exr()
        before = _state(r)
        assert L.de_environment_capture(h, -1) == ERR_INVALID and L.de_environment_capture(h, 6) == ERR_INVALID
        assert L.de_fetch_environment_face(h, 6, out.ctypes.data) == ERR_INVALID and _state(r) == before
        # a vignette and auto-exposure live behind the display: the capture succeeds, and is the same mean
        r.vignette_strength = 0.5
        r.set_auto_exposure(True)
        r.capture_environment_face(0)
        r.set_auto_exposure(False)
        r.vignette_strength = 0.0
        _same(r.fetch_environment_face(0), (r.fetch_hdr() / F(1)).astype(F), "under a vignette and auto-exposure")
        # five linear faces, then the EXR calls
        for face in range(1, 5):
            r.capture_environment_face(face)
        before = _state(r)
        assert before[5] == (0, 1, 2, 3, 4)
        n = ctypes.c_uint64()
        room = ctypes.create_string_buffer(b"\xA5" * 64, 64)
        assert L.de_render_to_exr(h, None, None) == ERR_STATE and L.de_fetch_exr_begin(h) == ERR_STATE
        assert L.de_fetch_exr(h, room, ctypes.c_uint64(64), ctypes.byref(n)) == ERR_STATE and room.raw == b"\xA5" * 64
        with pytest.raises(R.DigitalEarthError) as e:
            r.fetch_exr()
        assert e.value.code == ERR_STATE and "de_environment_capture" in str(e.value) and _state(r) == before
        r.reset_framebuffer()                                       # de_reset keeps the slots
        r.accumulate(1)
        r.capture_environment_face(5)
        full = r.fetch_exr()
        assert exr.read(full)[0].shape == (32, 64, 3)
        # AOV channels do not exist in this mode
        r.set_exr(aovs=("depth",))
        before = _state(r)
        with pytest.raises(R.DigitalEarthError) as e:
            r.fetch_exr()
        assert e.value.code == ERR_STATE and "AOV" in str(e.value) and L.de_fetch_exr_begin(h) == ERR_STATE and _state(r) == before
        r.set_exr()
        _same_bytes(r.fetch_exr(), full, "after the AOV refusal")
        # de_set_panorama while a fetch of the environment is in flight
        assert r.fetch_exr(lag=1) is None
        before = _state(r)
        with pytest.raises(R.DigitalEarthError) as e:
            r.set_panorama((48, 24))
        assert e.value.code == ERR_STATE and _state(r) == before
        _same_bytes(r.fetch_pending_exr(), full, "the fetch that was in flight")
        # a panorama beyond the EXR output's limit, width height 3 bps <= 2^27: 6144 x 2048 fits at half, not at float
        r.set_panorama((6144, 2048), supersample=1)
        assert r.environment["captured"] == ()                      # every set clears the linear slots with its own
        for face in range(6):
            r.capture_environment_face(face)
        r.set_exr(pixel_type="float")
        before = _state(r)
        with pytest.raises(R.DigitalEarthError) as e:
            r.fetch_exr()
        assert e.value.code == ERR_INVALID and L.de_fetch_exr_begin(h) == ERR_INVALID and _state(r) == before
        cap = ctypes.c_uint64(5)
        assert L.de_exr_capacity(h, ctypes.byref(cap)) == ERR_INVALID and cap.value == 5
    finally:
        _off(r)
    # the stage off again: the pinhole file's bytes as before
    assert r.environment["captured"] == ()
    _same_bytes(r.fetch_exr(), pinhole, "the stage off again")


# ---------------------------------------------------------------- 6. the viewer
def test_earth_viewer_frames_records_and_saves_the_environment(tmp_path):
    from digital_earth_amd.earth_viewer import EarthViewer
    v = EarthViewer(screen_res=(N, N), panorama=dict(size=(64, 32), supersample=1), **SCENE)
    got = v.frame(spp=1, panorama=True, exr=True)
    back, info = exr.read(got)
    assert isinstance(got, bytes) and back.shape == (32, 64, 3) and back.dtype == np.float16 and float(back.max()) > 0.0
    pattern = str(tmp_path / "env%05d.exr")
    assert v.record(pattern, 2, panorama=True) == 2
    for k in range(2):
        assert exr.read(open(pattern % k, "rb").read())[0].shape == (32, 64, 3)
    assert v.finish_exr() is None
    path = str(tmp_path / "x.exr")
    v.save(path)
    _same_bytes(open(path, "rb").read(), v.renderer.fetch_exr(), "save writes what fetch_exr delivers")
    assert exr.read(open(path, "rb").read())[0].shape == (32, 64, 3)
    v.close()
