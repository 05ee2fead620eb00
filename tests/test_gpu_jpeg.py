"""The JPEG output (include/digital_earth_jpeg.h) on the GPU: the stream of the four kernels equals the numpy restatement
(tests/jpeg_ref.py) byte for byte, on the sizes and inputs of tests/jpeg_cases.py through de_debug_jpeg and end to end behind the unchanged display
transform, a look and output scaling; the synchronous fetch, the view, the ring at every lag and EarthViewer deliver that stream; the other fetches
are untouched before, during and after; nothing is allocated until the feature is used; every error answers its code."""
import ctypes
import io

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_ref as jr

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = -1, -4
W, H = 64, 32


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    r.copy_textures()
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _sums(seed=0, W=W, H=H):
    rng = np.random.default_rng(7 + seed)
    s = (np.exp2(rng.uniform(-9.0, 3.0, (W, H, 1))) * rng.uniform(0.3, 1.6, (W, H, 3))).astype(F)
    s[: W // 4, : H // 4] = 0.0
    return s


def _same(got, want, what=""):
    got, want = bytes(got), bytes(want)
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("%s: %d bytes against %d, first difference at %d" % (what, len(got), len(want), first))


# ---------------------------------------------------------------- 1. the kernels, byte for byte
@pytest.mark.parametrize("size", jc.SIZES, ids=lambda s: "%dx%d-r%d" % s)
def test_stream_equals_the_restatement(ctx, size):
    w, h, restart = size
    before = ctx.jpeg()
    for name in jc.INPUTS:
        jc.check_precondition(name, w, h, restart)
        got = ctx.debug_jpeg(jc.image(name, w, h), quality=jc.QUALITY[name], restart=restart)
        _same(got, jc.reference(name, w, h, restart)[0], (name, size))
    assert ctx.jpeg() == before                                   # the debug entry point leaves the context's settings alone


# ---------------------------------------------------------------- 2. end to end on a context
def test_fetches_deliver_the_stream_of_fetch_image(R, ctx):
    r = ctx
    r.upload_hdr(_sums(), 3)
    assert r.jpeg() == dict(quality=90, restart=jr.DEFAULT_RESTART, size=(W, H), capacity=jr.capacity(W, H, jr.DEFAULT_RESTART))
    for quality, restart in ((90, None), (35, 1), (100, 3)):
        r.set_jpeg(quality, restart)
        shown = r.fetch_image()
        want = r.debug_jpeg(shown, quality=quality, restart=restart)
        _same(want, jr.encode(shown, quality, restart), "the debug entry point on the displayed image")
        got = r.fetch_jpeg()
        assert isinstance(got, bytes)
        _same(got, want, ("fetch_jpeg", quality))
        view = r.fetch_jpeg(copy=False)
        assert isinstance(view, memoryview) and view.readonly
        _same(view, want, "the view")
        del view
        assert r.jpeg()["capacity"] >= len(want)
    p, n = r.render_to_jpeg()
    assert p and n and p - n == 16                                 # the length stands 16 bytes in front of the stream
    Image = pytest.importorskip("PIL.Image")
    im = Image.open(io.BytesIO(got))
    im.load()
    assert im.size == (W, H)
    r.set_jpeg()


def test_stream_follows_the_look_and_output_scaling(ctx):
    r = ctx
    r.upload_hdr(_sums(1), 2)
    plain = r.fetch_jpeg()
    from digital_earth_amd.cube import Cube
    grid = np.linspace(0.0, 1.0, 5, dtype=F)
    b, g, red = np.meshgrid(grid, grid, grid, indexing="ij")       # file order: red fastest
    r.set_look(cube=Cube("3d", 5, (1.0 - np.stack([red, g, b], axis=-1)).astype(F)))      # a negative
    r.set_output_scale((48, 40), filter="mitchell")                # H = 8 mod 16
    try:
        shown = r.fetch_image()
        assert shown.shape == (48, 40, 3)
        got = r.fetch_jpeg()
        _same(got, jr.encode(shown, 90, None), "behind the look and output scaling")
        assert got != plain and r.jpeg()["size"] == (48, 40)
        assert r.fetch_jpeg(lag=1) is None
        _same(r.fetch_pending_jpeg(), got, "the ring at the output size")
    finally:
        r.set_output_scale(None)
        r.set_look(enabled=False)
    _same(r.fetch_jpeg(), plain, "back to the plain frame")


@pytest.mark.parametrize("lag", (1, 2, 3))
def test_ring_hands_out_every_frame_in_order(ctx, lag):
    r = ctx
    r.set_jpeg(92, 2)
    want, got = [], []
    for k in range(6):
        r.upload_hdr(_sums(10 + k), 1 + k % 2)
        want.append(r.debug_jpeg(r.fetch_image(), quality=92, restart=2))
        out = r.fetch_jpeg(lag=lag)
        assert (out is None) == (k < lag)
        if out is not None:
            got.append(out)
    with pytest.raises(RuntimeError):
        r.fetch_jpeg()                                             # a synchronous fetch while lagged ones are in flight
    got += r.fetch_pending_jpeg(all_images=True)
    assert len(got) == 6 and len({bytes(g) for g in got}) == 6
    for k in range(6):
        _same(got[k], want[k], ("lag", lag, "frame", k))
    assert r.fetch_pending_jpeg() is None
    r.set_jpeg()


def test_other_fetches_are_untouched_and_nothing_allocates_unused(R):
    W, H = 512, 256                                                # large enough for its buffers (2 x 1.3 MB on the device) to show in the counter
    hip = ctypes.CDLL("libamdhip64.so")                            # the runtime the library itself runs on: its count of free device memory

    def free_bytes():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    r.copy_textures()
    r.upload_hdr(_sums(3, W, H), 3)
    r.set_pixels(3, "round")
    r.set_video("i420", "bt601", "full", "center")

    def others():
        return _bits(r.fetch_image()).copy(), r.fetch_pixels().copy(), r.fetch_video().copy()
    before = others()
    for lag in (1, 1):                                             # warm every other ring too
        r.fetch_image(lag=lag), r.fetch_pixels(lag=lag), r.fetch_video(lag=lag)
    r.fetch_pending(), r.fetch_pending(pixels=True), r.fetch_pending(video=True)
    free0 = free_bytes()
    again = others()
    assert free_bytes() == free0                                   # with set_jpeg never called, nothing allocates
    for a, b in zip(before, again):
        assert (a == b).all()
    want = r.fetch_jpeg()
    assert free_bytes() < free0                                    # the first use does
    # during: JPEG fetches in flight beside the three other rings
    assert r.fetch_jpeg(lag=2) is None and r.fetch_jpeg(lag=2) is None
    assert r.fetch_image(lag=1) is None and r.fetch_pixels(lag=1) is None and r.fetch_video(lag=1) is None
    during = (_bits(r.fetch_pending()), r.fetch_pending(pixels=True), r.fetch_pending(video=True))
    for a, b in zip(before, during):
        assert (a == np.asarray(b)).all()
    for a, b in zip(before, others()):
        assert (a == b).all()
    for out in r.fetch_pending_jpeg(all_images=True):
        _same(out, want, "a frame fetched beside the other rings")
    for a, b in zip(before, others()):                             # after
        assert (a == b).all()
    r.close()


def test_every_error_answers_its_code(R, ctx):
    r = ctx
    L, h = r._lib, r._h
    r.upload_hdr(_sums(4), 1)
    before = r.jpeg()
    for kw in (dict(quality=0), dict(quality=101), dict(restart=0), dict(restart=65536)):
        with pytest.raises(R.DigitalEarthError) as e:
            r.set_jpeg(**kw)
        assert e.value.code == ERR_INVALID and r.jpeg() == before
    s = R.DeJpeg()
    s.struct_bytes, s.quality, s.restart_mcus = 8, 90, 8
    assert L.de_set_jpeg(h, ctypes.byref(s)) == ERR_INVALID and r.jpeg() == before
    assert r.fetch_jpeg(lag=1) is None
    with pytest.raises(R.DigitalEarthError) as e:
        r.set_jpeg(50)                                             # while a JPEG fetch is in flight
    assert e.value.code == ERR_STATE and r.jpeg() == before
    with pytest.raises(R.DigitalEarthError) as e:
        r.set_output_scale((48, 40))
    assert e.value.code == ERR_STATE
    for _ in range(3):
        assert L.de_fetch_jpeg_begin(h) == 0
        r._jp_in_flight += 1
    assert L.de_fetch_jpeg_begin(h) == ERR_STATE                   # a fifth
    assert len(r.fetch_pending_jpeg(all_images=True)) == 4
    ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    assert L.de_fetch_jpeg_end(h, ctypes.byref(ptr), ctypes.byref(n)) == ERR_STATE      # an _end without a _begin
    full = r.fetch_jpeg()
    small = ctypes.create_string_buffer(b"\xA5" * 100, 100)
    assert L.de_fetch_jpeg(h, small, ctypes.c_uint64(100), ctypes.byref(n)) == ERR_INVALID and n.value == len(full) and small.raw == b"\xA5" * 100
    img = np.zeros((16, 16, 3), F)
    s.struct_bytes = 12
    assert L.de_debug_jpeg(h, img.ctypes.data, 15, 16, ctypes.byref(s), small, ctypes.c_uint64(100), ctypes.byref(n)) == ERR_INVALID       # an odd size
    assert L.de_debug_jpeg(h, img.ctypes.data, 16, 16, ctypes.byref(s), small, ctypes.c_uint64(100), ctypes.byref(n)) == ERR_INVALID       # too small an `out` ...
    assert n.value == len(jr.encode(img, 90, 8)) and small.raw == b"\xA5" * 100                                                            # ... with the length set
    _same(r.fetch_jpeg(), full, "after the refusals")


def test_earth_viewer_frames_saves_and_records(tmp_path):
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(W, H), texture_source="synthetic", texture_size=(1024, 512), seed=5)
    a, d, c = EarthViewer(**kw), EarthViewer(**kw), EarthViewer(**kw)
    r = d.renderer
    for v in (d, c):
        v.renderer.set_jpeg(80, 2)
    for bad in (dict(pixels=True), dict(hdr_pixels=True), dict(video=True)):
        with pytest.raises(ValueError):
            d.frame(spp=1, jpeg=True, **bad)
    floats = [a.frame(spp=1).copy() for k in range(3)]
    got = [d.frame(spp=1, jpeg=True) for k in range(3)]
    for k in range(3):
        assert isinstance(got[k], bytes)
        _same(got[k], r.debug_jpeg(floats[k], 80, 2), ("frame(jpeg=True)", k))
    piped = [c.frame(spp=1, pipelined=1, jpeg=True) for k in range(3)]
    assert piped[0] is None
    _same(piped[1], got[0]); _same(piped[2], got[1]); _same(c.finish(jpeg=True), got[2])
    assert c.finish(jpeg=True) is None
    a.close(); c.close()
    img = d.frame(spp=1)
    path = str(tmp_path / "x.jpg")
    d.save(path)
    _same(open(path, "rb").read(), r.debug_jpeg(img, 80, 2), "save('x.jpg')")
    from digital_earth_amd import mjpeg     # noqa: F401
    avi = str(tmp_path / "fly.avi")
    assert d.record(avi, 5, sun_angle=[0.2, 0.4, 0.6, 0.8, 1.0]) == 5
    data = open(avi, "rb").read()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and data.count(b"00dc") >= 10 and int.from_bytes(data[4:8], "little") == len(data) - 8
    raw = str(tmp_path / "fly.mjpeg")
    assert d.record(raw, 3) == 3
    body = open(raw, "rb").read()
    assert body[:2] == b"\xff\xd8" and body.count(b"\xff\xd8\xff\xe0") == 3 and body[-2:] == b"\xff\xd9"
    d.close()
