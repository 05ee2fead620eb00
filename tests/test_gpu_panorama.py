"""The panorama stage (include/digital_earth_panorama.h) on the GPU: the kernel equals the numpy restatement (tests/panorama_ref.py)
bit for bit with the device's own de_sincos and square root handed to it, on random faces through de_debug_panorama and end to end behind six real
renders; the packed and coded outputs deliver the panorama's size and equal their own references on that image; the orientation of every face is
held to the float64 sphere; a context that turns the stage off again returns the bytes it always returned; every refusal answers its code.

Shapes, the smallest at which each thing can go wrong: faces of N = 16 (de_create's smallest square); 64 x 32 equirect (two whole tiles), 48 x 24
equirect (a partial 32 x 32 tile on both axes), 32 x 32 fisheye at 180° (five faces) and 360° (six, the pole at the rim); S = 1, 2, 3 (3: a
sub-position count that is no power of two); aprons 1 and 4 (the largest N / 4 admits); the world axes and an oblique frame.  More than one tile
along the second axis (panorama_ref.MULTI_TILE): 96 x 40 and 48 x 72 equirect (3 x 2 and 2 x 3 tiles, the last partial), 48 x 48 fisheye at 90° and
80 x 80 at 220° (2 x 2 and 3 x 3, partial), S = 1, 3, 4 (4: the LDS tables full), and faces of N = 40 with apron 10 beside N = 16.  The same shapes
with faces of a linear content against its float64 closed form: the kernel's image held to something not written from the header."""
import ctypes

import numpy as np
import pytest

import panorama_ref as ref
import pixels_ref as px

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = -1, -4
N = 16
OUTPUTS = [((64, 32), "equirect", 180.0), ((48, 24), "equirect", 180.0), ((32, 32), "fisheye", 180.0), ((32, 32), "fisheye", 360.0)]
APRONS = (1, 4)
SUPERSAMPLES = (1, 2, 3)
_f = np.array([2.0, -1.0, 2.0]) / 3.0
_u = np.array([1.0, 2.0, 0.0]) / np.sqrt(5.0)
_u = _u - _f * (_u @ _f)
_u /= np.linalg.norm(_u)
OBLIQUE = np.stack([np.cross(_f, _u), _u, _f])      # rows r, u, f with r = f x u, as the renderer's right, up, forward
RADIUS = 6371e3


def random_faces(n, seed):
    return np.random.default_rng(1000 + seed).random((6, n, n, 3), dtype=F)


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    """One square Renderer on small synthetic maps, shared by every test."""
    r = R.Renderer((N, N), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512))
    r.copy_textures()
    yield r
    r.close()


def device_leaves(r):
    """The device's de_sincos (de_debug_math 2 and 3 are its two outputs) and its square root (8), for the restatement."""
    return (lambda x: (r.debug_math(2, x), r.debug_math(3, x))), (lambda x: r.debug_math(8, x))


def _same(got, want, what=""):
    assert got.dtype == F and got.shape == want.shape, (what, got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


# ---------------------------------------------------------------- 5. the kernel, bit for bit
@pytest.mark.parametrize("output", OUTPUTS)
def test_kernel_equals_the_restatement_bit_for_bit(ctx, output):
    size, projection, aperture = output
    sincos, sqrt = device_leaves(ctx)
    held = ctx.panorama
    for apron in APRONS:
        for S in SUPERSAMPLES:
            for basis in (None, OBLIQUE):
                faces = random_faces(N, seed=S + 10 * apron)
                got = ctx.debug_panorama(faces, size, projection, aperture, apron, S, basis)
                want = ref.panorama(faces, size, projection, aperture, apron, S, basis, sincos=sincos, sqrt=sqrt)
                _same(got, want, (output, apron, S, basis is not None))
                assert got.min() >= 0.0 and got.max() < 1.0 and len(np.unique(got)) > got.size // 8      # a picture of the faces, not a flat field
    now = ctx.panorama
    assert now["on"] == held["on"] and now["size"] == held["size"] and now["captured"] == held["captured"]      # the debug entry point leaves the context alone
    odd = random_faces(5, seed=7)                                   # any n >= 4: de_create's size rule does not bind the debug entry point
    _same(ctx.debug_panorama(odd, size, projection, aperture, 1, 2), ref.panorama(odd, size, projection, aperture, 1, 2, sincos=sincos, sqrt=sqrt), "n = 5")


@pytest.mark.parametrize("output", ref.MULTI_TILE)
def test_kernel_equals_the_restatement_on_more_than_one_tile_per_axis(ctx, output):
    """Outputs of 3 x 2, 2 x 3, 2 x 2 and 3 x 3 tiles, the last tile partial (tests/test_panorama_ref.py states in numpy what each reaches): the tile
    decode's / and %, the latitude tables' base j0 S and their [b][jl] layout, the in_i and in_j guards, and the fisheye's ki, kj beyond the first
    tile.  S = 4 fills the LDS tables to their 128 entries on random faces; N = 40 with apron 10 is a face larger than a tile whose rows are 120 floats."""
    size, projection, aperture = output
    sincos, sqrt = device_leaves(ctx)
    for n, apron in ref.FACE_SIZES:
        for S in (1, 3, 4):
            for basis in (None, OBLIQUE):
                faces = random_faces(n, seed=S + 10 * apron + n)
                got = ctx.debug_panorama(faces, size, projection, aperture, apron, S, basis)
                want = ref.panorama(faces, size, projection, aperture, apron, S, basis, sincos=sincos, sqrt=sqrt)
                _same(got, want, (output, n, apron, S, basis is not None))
                assert got.min() >= 0.0 and got.max() < 1.0 and len(np.unique(got)) > got.size // 8


@pytest.mark.parametrize("S", (1, 4))
@pytest.mark.parametrize("output", ref.MULTI_TILE + [((32, 32), "fisheye", 360.0)])
def test_linear_faces_come_out_as_the_float64_direction_field_on_the_device(ctx, output, S):
    """The one comparison of the kernel with something that is not written from the header: faces whose content is linear in (u, v), built from the
    float64 face cameras alone (ref.f64_linear_faces), come out at every pixel inside the image as D / max |component of D| of the pixel's float64
    direction D (at S = 4: the mean over the sixteen sub-positions, a 0 for each beyond the fisheye's circle), and as exactly 0 outside.  The bound is
    the CPU test's (tests/test_panorama_ref.py): four times the restatement's own largest error, 2.28e-6 at S = 1 and 1.64e-6 at S = 4, where a
    transposed or half-pixel-shifted tap errs by 0.07."""
    size, projection, aperture = output
    worst = 0.0
    for apron in APRONS:
        for basis in (None, OBLIQUE):
            got = ctx.debug_panorama(ref.f64_linear_faces(N, apron, basis), size, projection, aperture, apron, S, basis)
            want, inside, outside = ref.f64_linear_image(size, projection, aperture, basis, S)
            assert got.dtype == F and got.shape == want.shape and inside.sum() > inside.size // 2
            assert (got[outside] == 0).all(), (output, S, apron)
            assert outside.any() == (projection == "fisheye") and (inside | outside).all() == (projection == "equirect" or S == 1)
            err = float(np.abs(got.astype(np.float64) - want)[~outside].max())
            print("linear field on the device %s S %d apron %d %s: max error %.3e" % (output, S, apron, "oblique" if basis is not None else "axes", err))
            worst = max(worst, err)
    assert 0.0 < worst <= ref.LINEAR_BOUND[S], (worst, ref.LINEAR_BOUND[S])      # 4 x ref.LINEAR_MEASURED[S], the restatement alone on the CPU


def test_constant_faces_survive_exactly_on_the_device(ctx):
    for size, projection, aperture in OUTPUTS:
        for S in (1, 2, 3, 4):
            for value in (0.0, 1.0, 0.3):
                got = ctx.debug_panorama(np.full((6, N, N, 3), value, F), size, projection, aperture, 1, S, OBLIQUE)
                vals = np.unique(got.view(np.uint32))
                if projection == "equirect":
                    assert vals.tolist() == [int(F(value).view(np.uint32))], (size, S, value)
                else:
                    assert got.min() >= 0.0 and got.max() == F(value) and got[16, 16, 0] == F(value) and got[0, 0, 0] == 0.0


# ---------------------------------------------------------------- 6. end to end
def _camera(r):
    r.set_camera_pos(-5.5e6, 1.0e6, 5.5e6)                          # 1.23 planet radii from the centre: the disc spans 108°, several faces see it
    r.set_look_at(0.0, 0.0, 0.0)
    r.set_up(0.0, 1.0, 0.0)
    r.set_fov(0.4)
    r.set_aspect_scale(1.0)
    r.vignette_strength = 0.0                                       # the reference's default vignette would print every face's border: captures refuse it


def _outputs(r):
    r.set_pixels(3, "round")
    r.set_jpeg(80)
    r.set_png()
    return r.fetch_image().copy(), r.fetch_pixels().copy(), bytes(r.fetch_png()), bytes(r.fetch_jpeg())


def test_end_to_end_six_renders_and_every_output(R, ctx):
    import jpeg_ref as jr
    import png_ref as pr
    r = ctx
    _camera(r)
    r.reset_framebuffer()
    r.accumulate(2)
    before = _outputs(r)                                            # the stage was never set on this context
    assert before[0].shape == (N, N, 3) and r.output_size() == (N, N)
    size = (64, 32)
    r.set_panorama(size, apron=1, supersample=2)
    assert r.output_size() == size and r.panorama["captured"] == ()
    r.render_panorama(2)
    p = r.panorama
    assert p["captured"] == (0, 1, 2, 3, 4, 5) and p["on"] and p["size"] == size
    basis = p["basis"]
    assert np.abs(basis.astype(np.float64) - r.camera_basis()).max() < 1e-6       # the caller's camera is back, and it was the default frame
    shown = r.fetch_image()
    assert shown.shape == size + (3,)
    assert np.allclose(tuple(r._params.look_at), (0.0, 0.0, 0.0)) and abs(r.fov[None] - 0.4) < 1e-7 and r.current_spp == 0
    pixels, png, jpeg = r.fetch_pixels(), r.fetch_png(), r.fetch_jpeg()
    assert pixels.shape == (size[1], size[0], 3)
    assert np.array_equal(pixels, px.pack(shown, 3, "round", 0, 0))
    back, _ = pr.decode(png)
    assert np.array_equal(back, pixels) and bytes(png) == bytes(pr.encode(pixels))
    assert bytes(jpeg) == bytes(jr.encode(shown, 80, None))
    view = r.fetch_image(copy=False)
    assert view.shape == size + (3,) and (np.array(view).view(np.uint32) == shown.view(np.uint32)).all()
    del view
    # the six faces beside it, with the stage off: the same cameras, the same seeds, fetch_image()
    r.set_panorama(size, apron=1, supersample=2, basis=basis, on=False)
    assert r.output_size() == (N, N)
    faces = np.empty((6, N, N, 3), F)
    for face in range(6):
        cam = r.panorama_face_camera(face)
        r.set_look_at(*cam["look_at"]); r._params.up[0], r._params.up[1], r._params.up[2] = cam["up"]; r._push_params()
        r.set_fov(cam["fov"]); r.set_aspect_scale(1.0)
        r.reset_framebuffer()
        r.accumulate(2)
        faces[face] = r.fetch_image()
    assert any(len(np.unique(faces[k])) > 8 for k in range(6)) and len(np.unique(shown)) > 64      # a picture, not a flat field (the faces that look away from the planet see black space)
    sincos, sqrt = device_leaves(r)
    _same(shown, ref.panorama(faces, size, "equirect", 180.0, 1, 2, basis, sincos=sincos, sqrt=sqrt), "fetch_image with the stage on")
    # off again: every call returns what it returned before the stage was ever set
    _camera(r)
    r.reset_framebuffer()
    r.accumulate(2)
    after = _outputs(r)
    assert (after[0].view(np.uint32) == before[0].view(np.uint32)).all() and np.array_equal(after[1], before[1]) and after[2] == before[2] and after[3] == before[3]
    r.set_pixels(); r.set_jpeg()


# ---------------------------------------------------------------- 7. orientation, free of noise
@pytest.mark.parametrize("sign", (1.0, -1.0))
def test_every_face_is_oriented_as_the_float64_sphere(ctx, sign):
    """The planet as a disc: the first-hit masks of the six face cameras (the guides' land coverage: 1 where a ray of the pixel hits), resampled at
    S = 1.  Every output pixel that is exactly 1 lies inside the planet's angular radius asin(R / |pos|) around the centre direction, every one that
    is exactly 0 outside it, in float64 with a margin of two face pixels' angle; values strictly between are under 10 % of the frame
    (tests/test_panorama_ref.py holds the float64 sphere alone to the same cap)."""
    r = ctx
    centre = sign * np.ones(3) / np.sqrt(3.0)                       # along (r + u + f) / sqrt 3 of the world axes, then its opposite
    pos = -1.5 * RADIUS * centre
    held = r.land_height_scale
    r.land_height_scale = 0.0
    size = (64, 32)
    try:
        r.set_camera_pos(*pos)
        r.set_panorama(size, apron=1, supersample=1, basis=np.eye(3), on=False)
        masks = np.zeros((6, N, N, 3), F)
        for face in range(6):
            cam = r.panorama_face_camera(face)
            r.set_look_at(*cam["look_at"]); r._params.up[0], r._params.up[1], r._params.up[2] = cam["up"]; r._push_params()
            r.set_fov(cam["fov"]); r.set_aspect_scale(1.0)
            r.reset_framebuffer()
            masks[face] = (r.fetch_guides()[..., 0] > 0)[..., None]
        seen = [bool(0 < masks[f].mean() < 1) for f in range(6)]
        assert seen == ([True, False] * 3 if sign > 0 else [False, True] * 3)      # the limb crosses the three faces towards the planet; both signs: all six
        got = r.debug_panorama(masks, size, "equirect", 180.0, 1, 1, np.eye(3))[..., 0]
    finally:
        r.land_height_scale = held
    x, y = np.meshgrid(np.arange(size[0]) + 0.5, np.arange(size[1]) + 0.5, indexing="ij")
    d, _ = ref.f64_direction(x, y, size, "equirect")
    ang = np.arccos(np.clip(d @ centre, -1, 1))
    radius = np.arcsin(RADIUS / np.linalg.norm(pos))
    margin = 2.0 * (2.0 * (N / (N - 2.0)) / N)
    between = (got > 0) & (got < 1)
    print("orientation, centre %+d: %.2f %% strictly between 0 and 1, %d ones, %d zeros" % (sign, 100.0 * between.mean(), (got == 1).sum(), (got == 0).sum()))
    assert (got == 1).sum() > 100 and (got == 0).sum() > 1000
    assert (ang[got == 1] <= radius + margin).all()
    assert (ang[got == 0] >= radius - margin).all()
    assert between.mean() < 0.10


# ---------------------------------------------------------------- 8. refusals on the device
def test_refusals_on_the_device(R, ctx):
    r = ctx
    L, h = r._lib, r._h
    _camera(r)
    r.reset_framebuffer()
    r.accumulate(1)
    r.set_panorama((64, 32))
    # capture under each stage that would print the face's border into the picture
    for on, off in ((lambda: r.set_bloom(True), lambda: r.set_bloom(False)), (lambda: r.set_auto_exposure(True), lambda: r.set_auto_exposure(False)),
                    (lambda: r.set_local_exposure(True), lambda: r.set_local_exposure(False)), (lambda: r.set_history(True), lambda: r.set_history(False))):
        on()
        assert L.de_panorama_capture(h, 0) == ERR_STATE and r.panorama["captured"] == ()
        off()
    r.vignette_strength = 0.5
    assert L.de_panorama_capture(h, 0) == ERR_STATE and r.panorama["captured"] == ()
    r.vignette_strength = 0.0
    assert L.de_panorama_capture(h, 6) == ERR_INVALID and L.de_panorama_capture(h, -1) == ERR_INVALID
    # fetch with five faces
    for face in range(5):
        r.capture_panorama_face(face)
    assert r.panorama["captured"] == (0, 1, 2, 3, 4)
    out = np.full((64, 32, 3), 7.0, F)
    assert L.de_fetch_image(h, out.ctypes.data) == ERR_STATE and (out == 7.0).all()
    assert L.de_render_to_image(h, None) == ERR_STATE and L.de_fetch_image_begin(h) == ERR_STATE
    for call in (r.fetch_pixels, r.fetch_png, r.fetch_jpeg, r.fetch_video, r.fetch_exr):
        with pytest.raises(R.DigitalEarthError) as e:
            call()
        assert e.value.code == ERR_STATE, call
    assert r.output_size() == (64, 32)
    r.reset_framebuffer()                                           # de_reset keeps the slots: the host resets between faces
    r.accumulate(1)
    assert r.panorama["captured"] == (0, 1, 2, 3, 4)
    r.capture_panorama_face(5)
    assert r.fetch_image().shape == (64, 32, 3)
    with pytest.raises(R.DigitalEarthError) as e:
        r.fetch_exr()                                               # the EXR output sits in front of the display
    assert e.value.code == ERR_STATE
    # output scaling and the panorama refuse each other
    with pytest.raises(R.DigitalEarthError) as e:
        r.set_output_scale((32, 16))
    assert e.value.code == ERR_STATE and r.output_size() == (64, 32) and r.output_scale()["on"] is False
    held = r.panorama
    assert L.de_fetch_image_begin(h) == 0                           # a lagged fetch in flight
    with pytest.raises(R.DigitalEarthError) as e:
        r.set_panorama((48, 24))
    assert e.value.code == ERR_STATE and r.panorama["size"] == held["size"] and r.panorama["captured"] == held["captured"]
    fp = ctypes.POINTER(ctypes.c_float)()
    assert L.de_fetch_image_end(h, ctypes.byref(fp)) == 0
    r.set_panorama((48, 24))                                        # every set clears the slots
    assert r.panorama["captured"] == () and r.output_size() == (48, 24)
    r.set_panorama((48, 24), on=False)
    r.set_output_scale((32, 16))
    with pytest.raises(R.DigitalEarthError) as e:
        r.set_panorama((64, 32))
    assert e.value.code == ERR_STATE and r.output_size() == (32, 16) and r.panorama["on"] is False
    r.set_output_scale(on=False)
    with pytest.raises(R.DigitalEarthError) as e:
        r.capture_panorama_face(0)                                  # the stage is off
    assert e.value.code == ERR_STATE
    # a context that is not square
    wide = R.Renderer((32, 16), (0, 1, 0), texture_source="constant")
    with pytest.raises(R.DigitalEarthError) as e:
        wide.set_panorama((64, 32))
    assert e.value.code == ERR_INVALID and wide.output_size() == (32, 16)
    wide.close()


def test_earth_viewer_frames_and_saves_the_panorama(tmp_path):
    from digital_earth_amd.earth_viewer import EarthViewer
    v = EarthViewer(screen_res=(N, N), texture_source="synthetic", texture_size=(1024, 512), panorama=dict(size=(64, 32), supersample=1))
    img = v.frame(spp=1, panorama=True)
    assert img.shape == (64, 32, 3) and len(np.unique(img)) > 16
    pix = v.frame(spp=1, pixels=True, panorama=True)
    assert pix.shape == (32, 64, 4)
    v.frame(spp=1, panorama=True)
    v.save(str(tmp_path / "pano.npy"))
    assert np.load(str(tmp_path / "pano.npy")).shape == (64, 32, 3)
    v.renderer.set_video("i420")
    assert v.record(str(tmp_path / "pano.y4m"), 2, spp=1, panorama=True) == 2
    assert b"W64 H32" in open(str(tmp_path / "pano.y4m"), "rb").read(40)
    v.close()
