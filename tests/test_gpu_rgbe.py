"""The Radiance HDR output (include/digital_earth_rgbe.h) on the GPU: the file of the four kernels equals the numpy restatement
(tests/rgbe_ref.py) byte for byte on the cases of tests/rgbe_cases.py through de_debug_rgbe; a context's file is the restatement's of
fetch_hdr() / spp; the ring hands out the synchronous fetch's bytes and refuses a fifth; the scene-linear panorama comes out as the restatement's
file of the image the EXR output delivers for the same slots; the other fetches are untouched.  Every comparison is of bytes."""
import ctypes

import numpy as np
import pytest

import rgbe_cases as gc
import rgbe_ref as gr
from digital_earth_amd import exr, rgbe

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = -1, -4
W, H = 64, 48
SCENE = dict(texture_source="synthetic", texture_size=(1024, 512))


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    r = R.Renderer((W, H), (0, 1, 0), **SCENE)
    r.copy_textures()
    r.accumulate(2)
    yield r
    r.close()


def _same(got, want, what=""):
    got, want = bytes(got), bytes(want)
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("%s: %d bytes against %d, first difference at %d" % (what, len(got), len(want), first))


def _oriented(field):
    """A (W, H, 3) field of the library -> (H, W, 3) rows top-down, as fetch_pixels orients the picture: file[r][x] = field[x][H - 1 - r]."""
    return np.ascontiguousarray(np.asarray(field)[:, ::-1].transpose(1, 0, 2))


# ---------------------------------------------------------------- 1. the kernels, byte for byte
@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_file_equals_the_restatement(ctx, name):
    image, rle, rounding, scale = gc.CASES[name]
    before = ctx.rgbe()
    got = ctx.debug_rgbe(image, rle=rle, rounding=rounding, scale=scale)      # (it also checks that nothing was written behind the file's length)
    _same(got, gc.encoded(name), name)
    assert len(got) <= gr.capacity(image.shape[1], image.shape[0], rle, scale)
    assert (b"EXPOSURE=0.25\n" in got[:200]) == (scale == 0.25)
    assert ctx.rgbe() == before                                    # the debug entry point leaves the context's settings alone


# ---------------------------------------------------------------- 2. end to end on a context
def test_context_file_is_fetch_hdr_over_spp(R, ctx):
    r = ctx
    r.set_rgbe()
    try:
        assert r.rgbe() == dict(source="mean", rle=True, rounding="trunc", scale=1.0, size=(W, H), capacity=gr.capacity(W, H))
        want = _oriented(r.fetch_hdr() / F(r.current_spp))
        assert want.dtype == F and r.current_spp == 2
        got = r.fetch_rgbe()
        assert isinstance(got, bytes)
        _same(got, gr.encode(want), "fetch_rgbe against the restatement on fetch_hdr / spp")
        assert np.array_equal(rgbe.decode(got)[0], gr.pixels(want))
        view = r.fetch_rgbe(copy=False)
        assert isinstance(view, memoryview) and view.readonly
        _same(view, got, "the view")
        del view
        p, n = r.render_to_rgbe()
        assert p and n and p - n == 16                             # the length stands 16 bytes in front of the file
        r.set_rgbe(rle=False, rounding="round", scale=0.5)
        _same(r.fetch_rgbe(), gr.encode(want, False, "round", 0.5), "flat, rounded, scale 0.5")
        r.set_rgbe(source="bloom")
        with pytest.raises(R.DigitalEarthError) as mine:
            r.fetch_rgbe()                                         # the stage is off: the EXR output's refusal, word for word
        r.set_exr(source="bloom")
        with pytest.raises(R.DigitalEarthError) as theirs:
            r.fetch_exr()
        assert mine.value.code == theirs.value.code == ERR_STATE and str(mine.value) == str(theirs.value)
    finally:
        r.set_rgbe()
        r.set_exr()


def test_ring_runs_four_deep_and_refuses_a_fifth(R, ctx):
    r = ctx
    L, h = r._lib, r._h
    r.set_rgbe()
    before = r.rgbe()
    full = r.fetch_rgbe()
    assert r.fetch_rgbe(lag=1) is None
    with pytest.raises(R.DigitalEarthError) as e:
        r.set_rgbe(rounding="round")                               # while an RGBE fetch is in flight
    assert e.value.code == ERR_STATE and r.rgbe() == before
    for _ in range(3):
        assert L.de_fetch_rgbe_begin(h) == 0
        r._rg_in_flight += 1
    assert L.de_fetch_rgbe_begin(h) == ERR_STATE                   # a fifth
    out = r.fetch_pending_rgbe(all_images=True)
    assert len(out) == 4
    for o in out:
        _same(o, full, "a lagged fetch of the same frame")
    ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    assert L.de_fetch_rgbe_end(h, ctypes.byref(ptr), ctypes.byref(n)) == ERR_STATE      # an _end without a _begin
    small = ctypes.create_string_buffer(b"\xA5" * 40, 40)
    assert L.de_fetch_rgbe(h, small, ctypes.c_uint64(40), ctypes.byref(n)) == ERR_INVALID and n.value == len(full) and small.raw == b"\xA5" * 40
    for kw in (dict(scale=0.0), dict(scale=float("inf")), dict(scale=float("nan"))):
        with pytest.raises(R.DigitalEarthError) as e:
            r.set_rgbe(**kw)
        assert e.value.code == ERR_INVALID and r.rgbe() == before
    for bad in (dict(source="image"), dict(rounding="even")):
        with pytest.raises(ValueError):
            r.set_rgbe(**bad)
    img = np.zeros((4, 4, 3), F)
    s = R.DeRgbe()
    s.struct_bytes, s.source, s.rle, s.rounding, s.scale = 20, 0, 1, 0, 1.0
    big = ctypes.create_string_buffer(4096)
    for w_, h_ in ((0, 4), (4, 0), (-1, 4), (1 << 13, (1 << 12) + 1)):
        assert L.de_debug_rgbe(h, img.ctypes.data, w_, h_, ctypes.byref(s), big, ctypes.c_uint64(4096), ctypes.byref(n)) == ERR_INVALID
    assert L.de_debug_rgbe(h, img.ctypes.data, 4, 4, ctypes.byref(s), small, ctypes.c_uint64(40), ctypes.byref(n)) == ERR_INVALID      # too small an `out` ...
    assert n.value == len(gr.encode(img)) and small.raw == b"\xA5" * 40                                                                 # ... with the length set
    _same(r.fetch_rgbe(), full, "after the refusals")


def test_lagged_fetches_deliver_the_synchronous_files_in_order(R):
    sync, r = (R.Renderer((W, H), (0, 1, 0), **SCENE) for _ in range(2))      # the same frames twice: one fetched synchronously, one through the ring
    want, got = [], []
    for x in (sync, r):
        x.copy_textures()
        x.set_rgbe()
    for k in range(5):
        sync.accumulate(1); r.accumulate(1)                        # the frames differ by one accumulate
        want.append(sync.fetch_rgbe())
        out = r.fetch_rgbe(lag=3)
        assert (out is None) == (k < 3)
        if out is not None:
            got.append(out)
    got += r.fetch_pending_rgbe(all_images=True)
    assert len(got) == 5 and len({bytes(g) for g in got}) == 5
    for k in range(5):
        _same(got[k], want[k], "frame %d" % k)
    sync.close(); r.close()


# ---------------------------------------------------------------- 3. the environment map
def test_environment_map_is_the_restatement_of_the_exr_outputs_image(R):
    N = 16
    r = R.Renderer((N, N), (0, 1, 0), seed=3, **SCENE)
    r.copy_textures()
    r.set_camera_pos(-5.5e6, 1.0e6, 5.5e6)
    r.set_look_at(0.0, 0.0, 0.0)
    r.set_fov(0.4)
    r.set_panorama((64, 32), supersample=1, basis=np.eye(3))
    r.set_rgbe(rounding="round")
    r.set_exr(pixel_type="float", compression="none")
    with pytest.raises(R.DigitalEarthError) as e:
        r.fetch_rgbe()                                             # no linear face yet
    assert e.value.code == ERR_STATE
    r.render_environment(1, basis=np.eye(3))
    image = exr.read(r.fetch_exr())[0]                             # the resampled slots as the EXR output delivers them: float32, top row first
    assert image.shape == (32, 64, 3) and image.dtype == F and len(np.unique(image)) > 64
    got = r.fetch_rgbe()
    _same(got, gr.encode(image, True, "round"), "the environment map")
    state = r.rgbe()
    assert state["size"] == (64, 32) and state["capacity"] == gr.capacity(64, 32) >= len(got)
    assert r.fetch_rgbe(lag=1) is None
    with pytest.raises(R.DigitalEarthError) as e:
        r.set_panorama((48, 24))                                   # while a fetch of the environment map is in flight
    assert e.value.code == ERR_STATE
    _same(r.fetch_pending_rgbe(), got, "the ring")
    faces = np.stack([r.fetch_environment_face(k) for k in range(6)])
    _same(r.debug_environment_rgbe(faces, (64, 32), supersample=1, basis=np.eye(3), rounding="round"), got, "de_debug_environment_rgbe on the same faces")
    r.set_panorama((64, 32), supersample=1, basis=np.eye(3))      # the masks are cleared ...
    for face in range(5):
        r.capture_environment_face(face)                           # ... and five slots are not six
    for call in (r.fetch_rgbe, lambda: r.fetch_rgbe(lag=1), r.render_to_rgbe, r.fetch_exr):
        with pytest.raises(R.DigitalEarthError) as e:
            call()
        assert e.value.code == ERR_STATE
    assert r._rg_in_flight == 0
    r.close()


# ---------------------------------------------------------------- 4. nothing moved
def test_a_context_that_never_sets_it_hands_out_the_same_bytes(R):
    a, b = (R.Renderer((W, H), (0, 1, 0), **SCENE) for _ in range(2))
    for x in (a, b):
        x.copy_textures()
        x.accumulate(2)
    a.set_rgbe(rounding="round", scale=2.0)
    first = a.fetch_rgbe()
    assert a.fetch_rgbe(lag=1) is None
    _same(a.fetch_exr(), b.fetch_exr(), "fetch_exr beside an RGBE fetch in flight")
    assert np.array_equal(a.fetch_image().view(np.uint32), b.fetch_image().view(np.uint32))
    _same(a.fetch_pending_rgbe(), first, "the ring beside the other fetches")
    a.set_rgbe()
    _same(a.fetch_exr(), b.fetch_exr(), "fetch_exr after it was unset")
    assert np.array_equal(a.fetch_image().view(np.uint32), b.fetch_image().view(np.uint32)) and np.array_equal(a.fetch_hdr().view(np.uint32), b.fetch_hdr().view(np.uint32))
    a.close(); b.close()


# ---------------------------------------------------------------- 5. the viewer
def test_earth_viewer_frames_saves_and_records(tmp_path):
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(W, H), seed=5, **SCENE)
    v = EarthViewer(**kw)
    path = str(tmp_path / "x.hdr")
    v.render(2)
    with pytest.raises(Exception) as never_set:
        v.save(path)                                               # set_rgbe() was never called: an extension the image writer does not know
    with pytest.raises(Exception) as unknown:
        v.save(str(tmp_path / "x.unknown_extension"))
    assert type(never_set.value) is type(unknown.value)
    v.renderer.set_rgbe()
    v.save(path)
    data = open(path, "rb").read()
    want = _oriented(v.renderer.fetch_hdr() / F(v.renderer.current_spp))
    _same(data, gr.encode(want), "save")
    stored = rgbe.decode(path)[0]
    step = np.ldexp(1.0, stored[..., 3:4].astype(np.int32) - 136)
    lit = np.broadcast_to(stored[..., 3:4] != 0, want.shape)
    held = np.maximum(want.astype(np.float64), 0.0)                # the source as the format can hold it: a negative component of the mean is 0
    assert (np.abs(rgbe.read(path)[0].astype(np.float64) - held) <= step)[lit].all()               # within one step, and with the half step within half of one
    assert (np.abs(rgbe.read(path, half_step=True)[0].astype(np.float64) - held) <= step / 2)[lit].all()
    for bad in (dict(pixels=True), dict(jpeg=True), dict(png=True), dict(exr=True)):
        with pytest.raises(ValueError):
            v.frame(spp=1, rgbe=True, **bad)
    v.renderer.reset_framebuffer()
    got = [v.frame(spp=1, rgbe=True) for k in range(2)]
    assert all(isinstance(g, bytes) for g in got) and got[0] != got[1] and rgbe.read(got[1])[0].shape == (H, W, 3)
    v.close()
    a, b = EarthViewer(**kw), EarthViewer(**kw)                    # one records, one shows the same frames
    pattern = str(tmp_path / "f%05d.hdr")
    angles = [0.2, 0.4, 0.6]
    assert a.record(pattern, 3, sun_angle=angles) == 3
    for k in range(3):
        _same(open(pattern % k, "rb").read(), b.frame(spp=1, rgbe=True, sun_angle=angles[k]), "recorded frame %d" % k)
    with pytest.raises(ValueError):
        a.record(str(tmp_path / "one.hdr"), 2)
    assert a.finish_rgbe() is None
    a.close(); b.close()
