"""The PNG output (include/digital_earth_png.h) on the GPU: the file of the four kernels equals the numpy restatement (tests/png_ref.py)
byte for byte on the cases of tests/png_cases.py through de_debug_png, and decodes to its input through an independent inflater; a rendered frame's
file decodes to exactly the packed pixels of the same frame, 8- and 16-bit, behind a look and output scaling; the ring hands out every frame in
order; the other fetches are untouched; nothing is allocated until the feature is used; every error answers its code."""
import ctypes

import numpy as np
import pytest

import png_cases as pc
import png_ref as pr

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = -1, -4
W, H = 64, 64


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
@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_stream_equals_the_restatement_and_decodes_to_the_input(ctx, name):
    px, flt, chunk = pc.CASES[name]
    before = ctx.png()
    got = ctx.debug_png(px, filter=flt, chunk_bytes=chunk)
    _same(got, pc.encoded(name)[0], name)
    back, info = pr.decode(got)
    assert back.dtype == px.dtype and np.array_equal(back, px)
    assert len(got) <= pr.capacity(px.shape[1], px.shape[0], px.shape[2], 8 * px.dtype.itemsize, chunk)
    assert ctx.png() == before                                     # the debug entry point leaves the context's settings alone


# ---------------------------------------------------------------- 2. end to end on a context
@pytest.mark.parametrize("channels", (3, 4))
@pytest.mark.parametrize("mode", ("truncate", "dither"))
def test_frame_decodes_to_fetch_pixels(ctx, channels, mode):
    r = ctx
    r.upload_hdr(_sums(channels), 3)
    r.set_pixels(channels, mode, seed=9)
    r.set_png()
    try:
        assert r.png() == dict(source="pixels", filter="adaptive", chunk_bytes=pr.DEFAULT_CHUNK, size=(W, H), capacity=pr.capacity(W, H, channels, 8))
        px = r.fetch_pixels().copy()
        got = r.fetch_png()
        assert isinstance(got, bytes)
        back, info = pr.decode(got)
        assert back.dtype == np.uint8 and np.array_equal(back, px) and info["cicp"] is None
        _same(got, pr.encode(px), "fetch_png against the restatement on fetch_pixels")
        view = r.fetch_png(copy=False)
        assert isinstance(view, memoryview) and view.readonly
        _same(view, got, "the view")
        del view
        p, n = r.render_to_png()
        assert p and n and p - n == 16                             # the length stands 16 bytes in front of the file
    finally:
        r.set_pixels()


def test_hdr_frame_decodes_to_fetch_hdr_pixels(R, ctx):
    r = ctx
    r.upload_hdr(_sums(5), 2)
    r.set_png(source="hdr_pixels", filter="paeth", chunk_bytes=2048)
    with pytest.raises(R.DigitalEarthError) as e:
        r.fetch_png()                                              # the HDR output is off
    assert e.value.code == ERR_STATE
    r.set_hdr_output(True, gamut="p3d65", transfer="hlg", pixel_format="rgb10a2")
    try:
        for call in (r.fetch_png, r.png, lambda: r.fetch_png(lag=1), r.render_to_png):
            with pytest.raises(R.DigitalEarthError) as e:
                call()                                             # RGB10A2 is no source
            assert e.value.code == ERR_STATE
        r.set_hdr_output(True, gamut="p3d65", transfer="hlg", pixel_format="rgb16", mode="round")
        px = r.fetch_hdr_pixels().copy()
        got = r.fetch_png()
        back, info = pr.decode(got)
        assert back.dtype == np.uint16 and np.array_equal(back, px) and info["cicp"] == bytes((12, 18, 0, 1))
        _same(got, pr.encode(px, "paeth", 2048, cicp=(12, 18, 0, 1)), "the 16-bit file against the restatement")
        r.set_png()                                                # the 8-bit source packs whatever signal the display wrote
        assert np.array_equal(pr.decode(r.fetch_png())[0], r.fetch_pixels())
    finally:
        r.set_hdr_output(False)
        r.set_png()


def test_file_follows_the_look_and_output_scaling(ctx):
    r = ctx
    r.upload_hdr(_sums(1), 2)
    r.set_png()
    plain = r.fetch_png()
    from digital_earth_amd.cube import Cube
    grid = np.linspace(0.0, 1.0, 5, dtype=F)
    b, g, red = np.meshgrid(grid, grid, grid, indexing="ij")
    r.set_look(cube=Cube("3d", 5, (1.0 - np.stack([red, g, b], axis=-1)).astype(F)))      # a negative
    r.set_output_scale((48, 40), filter="mitchell")
    try:
        px = r.fetch_pixels().copy()
        assert px.shape[:2] == (40, 48)
        got = r.fetch_png()
        assert np.array_equal(pr.decode(got)[0], px) and got != plain and r.png()["size"] == (48, 40)
        r.set_hdr_output(True, pixel_format="rgb16")
        r.set_png(source="hdr_pixels")
        assert np.array_equal(pr.decode(r.fetch_png())[0], r.fetch_hdr_pixels())
        r.set_hdr_output(False)
        r.set_png()
        assert r.fetch_png(lag=1) is None
        _same(r.fetch_pending_png(), got, "the ring at the output size")
    finally:
        r.set_hdr_output(False)
        r.set_png()
        r.set_output_scale(None)
        r.set_look(enabled=False)
    _same(r.fetch_png(), plain, "back to the plain frame")


@pytest.mark.parametrize("lag", (1, 2, 3))
def test_ring_hands_out_every_frame_in_order(R, lag):
    r = R.Renderer((W, H), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512))
    r.copy_textures()
    r.set_pixels(3, "round")
    r.set_png(chunk_bytes=4096)
    want, got = [], []
    for k in range(6):
        r.accumulate(1)                                            # the frames differ by one accumulate
        want.append(r.fetch_pixels().copy())
        out = r.fetch_png(lag=lag)
        assert (out is None) == (k < lag)
        if out is not None:
            got.append(out)
    with pytest.raises(RuntimeError):
        r.fetch_png()                                              # a synchronous fetch while lagged ones are in flight
    got += r.fetch_pending_png(all_images=True)
    assert len(got) == 6 and len({bytes(g) for g in got}) == 6
    for k in range(6):
        assert np.array_equal(pr.decode(got[k])[0], want[k]), (lag, k)
    assert r.fetch_pending_png() is None
    r.close()


def test_other_fetches_are_untouched_and_nothing_allocates_unused(R):
    W, H = 1024, 512                                               # large enough for its buffers (four of 1.5 MB on the device) to show in the counter
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
        return r.fetch_image().view(np.uint32).copy(), r.fetch_pixels().copy(), r.fetch_video().copy(), np.frombuffer(r.fetch_jpeg(), np.uint8)
    before = others()
    for lag in (1, 1):                                             # warm every other ring too
        r.fetch_image(lag=lag), r.fetch_pixels(lag=lag), r.fetch_video(lag=lag), r.fetch_jpeg(lag=lag)
    r.fetch_pending(), r.fetch_pending(pixels=True), r.fetch_pending(video=True), r.fetch_pending_jpeg()
    free0, use0 = free_bytes(), r.memory_use()
    again = others()
    assert free_bytes() == free0 and r.memory_use() == use0        # with no PNG call made, nothing allocates
    for a, b in zip(before, again):
        assert (a == b).all()
    r.set_png()
    assert free_bytes() == free0                                   # nor by the settings
    want = r.fetch_png()
    assert free_bytes() < free0                                    # the first use does
    _same(want, pr.encode(before[1]), "the first file against the restatement on fetch_pixels")
    assert r.fetch_png(lag=2) is None and r.fetch_png(lag=2) is None      # during: PNG fetches in flight beside the other rings
    assert r.fetch_image(lag=1) is None and r.fetch_pixels(lag=1) is None and r.fetch_video(lag=1) is None and r.fetch_jpeg(lag=1) is None
    during = (r.fetch_pending().view(np.uint32), r.fetch_pending(pixels=True), r.fetch_pending(video=True), np.frombuffer(r.fetch_pending_jpeg(), np.uint8))
    for a, b in zip(before, during):
        assert (a == np.asarray(b)).all()
    for out in r.fetch_pending_png(all_images=True):
        _same(out, want, "a frame fetched beside the other rings")
    for a, b in zip(before, others()):                             # after
        assert (a == b).all()
    r.close()


def test_every_error_answers_its_code(R, ctx):
    r = ctx
    L, h = r._lib, r._h
    r.upload_hdr(_sums(4), 1)
    r.set_png()
    before = r.png()
    for kw in (dict(chunk_bytes=1023), dict(chunk_bytes=65536)):
        with pytest.raises(R.DigitalEarthError) as e:
            r.set_png(**kw)
        assert e.value.code == ERR_INVALID and r.png() == before
    s = R.DePng()
    for fields in ((12, 0, 5, 16384), (16, 2, 5, 16384), (16, -1, 5, 16384), (16, 0, 6, 16384), (16, 0, -1, 16384)):
        s.struct_bytes, s.source, s.filter, s.chunk_bytes = fields
        assert L.de_set_png(h, ctypes.byref(s)) == ERR_INVALID and r.png() == before
    for bad in (dict(source="floats"), dict(filter="best")):
        with pytest.raises(ValueError):
            r.set_png(**bad)
    assert r.fetch_png(lag=1) is None
    with pytest.raises(R.DigitalEarthError) as e:
        r.set_png(filter="up")                                     # while a PNG fetch is in flight
    assert e.value.code == ERR_STATE and r.png() == before
    with pytest.raises(R.DigitalEarthError) as e:
        r.set_output_scale((48, 40))
    assert e.value.code == ERR_STATE
    for _ in range(3):
        assert L.de_fetch_png_begin(h) == 0
        r._pn_in_flight += 1
    assert L.de_fetch_png_begin(h) == ERR_STATE                    # a fifth
    assert len(r.fetch_pending_png(all_images=True)) == 4
    ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    assert L.de_fetch_png_end(h, ctypes.byref(ptr), ctypes.byref(n)) == ERR_STATE      # an _end without a _begin
    full = r.fetch_png()
    small = ctypes.create_string_buffer(b"\xA5" * 40, 40)
    assert L.de_fetch_png(h, small, ctypes.c_uint64(40), ctypes.byref(n)) == ERR_INVALID and n.value == len(full) and small.raw == b"\xA5" * 40
    px = np.zeros((4, 4, 3), np.uint8)
    s.struct_bytes, s.source, s.filter, s.chunk_bytes = 16, 0, 5, 16384
    big = ctypes.create_string_buffer(4096)
    for w_, h_, ch, depth in ((0, 4, 3, 8), (4, 0, 3, 8), (4, 4, 2, 8), (4, 4, 4, 16), (4, 4, 3, 12), (1 << 14, 1 << 12, 3, 8)):
        assert L.de_debug_png(h, px.ctypes.data, w_, h_, ch, depth, ctypes.byref(s), big, ctypes.c_uint64(4096), ctypes.byref(n)) == ERR_INVALID
    assert L.de_debug_png(h, px.ctypes.data, 4, 4, 3, 8, ctypes.byref(s), small, ctypes.c_uint64(40), ctypes.byref(n)) == ERR_INVALID      # too small an `out` ...
    assert n.value == len(pr.encode(px)) and small.raw == b"\xA5" * 40                                                                       # ... with the length set
    _same(r.fetch_png(), full, "after the refusals")


def test_earth_viewer_frames_saves_and_records(tmp_path):
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(W, H), texture_source="synthetic", texture_size=(1024, 512), seed=5)
    a, d, c = EarthViewer(**kw), EarthViewer(**kw), EarthViewer(**kw)
    r = d.renderer
    old = str(tmp_path / "old.png")
    d.render(1)
    d.save(old)                                                    # before set_png: the host writer's file
    a.render(1)
    a.save(str(tmp_path / "old_a.png"))
    assert open(old, "rb").read() == open(str(tmp_path / "old_a.png"), "rb").read()
    for v in (a, d, c):
        v.renderer.reset_framebuffer()
    for v in (d, c):
        v.renderer.set_png(chunk_bytes=2048)
    for bad in (dict(pixels=True), dict(hdr_pixels=True), dict(video=True), dict(jpeg=True)):
        with pytest.raises(ValueError):
            d.frame(spp=1, png=True, **bad)
    pixels = [a.frame(spp=1, pixels=True).copy() for k in range(3)]
    got = [d.frame(spp=1, png=True) for k in range(3)]
    for k in range(3):
        assert isinstance(got[k], bytes) and np.array_equal(pr.decode(got[k])[0], pixels[k]), k
    piped = [c.frame(spp=1, pipelined=1, png=True) for k in range(3)]
    assert piped[0] is None
    _same(piped[1], got[0]); _same(piped[2], got[1]); _same(c.finish_png(), got[2])
    assert c.finish_png() is None
    c.close()
    px = d.frame(spp=1, pixels=True).copy()
    path = str(tmp_path / "x.png")
    d.save(path)
    data = open(path, "rb").read()
    _same(data, pr.encode(px, "adaptive", 2048), "save('x.png') with PNG output set: the GPU's file")
    a.frame(spp=1, pixels=True)
    a.save(str(tmp_path / "a.png"))
    other = open(str(tmp_path / "a.png"), "rb").read()
    assert other != data and other.count(b"IDAT") == 1             # without set_png: the host writer, as before
    assert np.array_equal(pr.decode(other)[0][..., :3], px[..., :3])
    a.close()
    d2, e = EarthViewer(**kw), EarthViewer(**kw)                   # a fresh pair: one records, one shows the same frames as pixels
    d2.renderer.set_png()
    pattern = str(tmp_path / "f%03d.png")
    angles = [0.2, 0.4, 0.6, 0.8]
    assert d2.record(pattern, 4, sun_angle=angles) == 4
    for k in range(4):
        want = e.frame(spp=1, pixels=True, sun_angle=angles[k])
        assert np.array_equal(pr.decode(open(pattern % k, "rb").read())[0], want), k
    d2.close()
    with pytest.raises(ValueError):
        d.record(str(tmp_path / "one.png"), 2)
    d.close(); e.close()
