"""The OpenEXR output (include/digital_earth_exr.h) on the GPU: the file of the six kernels equals the numpy restatement
(tests/exr_ref.py) byte for byte on the cases of tests/exr_cases.py through de_debug_exr, and decodes through the independent reader
(digital_earth_amd/exr.py); a context's file decodes to exactly fetch_hdr() / spp, or to exactly the matching stage's fetch; the ring hands out the
synchronous fetch's bytes; the other fetches are untouched; every error answers its code."""
import ctypes

import numpy as np
import pytest

import exr_cases as xc
import exr_ref as xr
from digital_earth_amd import exr

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = -1, -4
W, H = 64, 64                                                      # the PNG tests' context: tests/test_gpu_png.py
SCENE = dict(texture_source="synthetic", texture_size=(1024, 512))


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    r = R.Renderer((W, H), (0, 1, 0), **SCENE)
    r.copy_textures()
    r.accumulate(3)
    yield r
    r.close()


def _same(got, want, what=""):
    got, want = bytes(got), bytes(want)
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("%s: %d bytes against %d, first difference at %d" % (what, len(got), len(want), first))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _oriented(field):
    """A (W, H, 3) field of the library -> (H, W, 3) rows top-down, as fetch_pixels orients the picture: file[r][x] = field[x][H - 1 - r]."""
    return np.ascontiguousarray(np.asarray(field)[:, ::-1].transpose(1, 0, 2))


# ---------------------------------------------------------------- 1. the kernels, byte for byte
@pytest.mark.parametrize("name", sorted(xc.CASES))
def test_file_equals_the_restatement_and_decodes(ctx, name):
    image, pixel_type, compression, chunk, scale = xc.CASES[name]
    before = ctx.exr()
    got = ctx.debug_exr(image, pixel_type=pixel_type, compression=compression, chunk_bytes=chunk, scale=scale)
    _same(got, xc.encoded(name)[0], name)
    back, info = exr.read(got)
    assert np.array_equal(_bits(back), _bits(xr.convert(image, scale, pixel_type)))
    assert [("raw" if b["raw"] else "zip") for b in info["blocks"]] == list(xc.encoded(name)[1])
    assert len(got) <= xr.capacity(image.shape[1], image.shape[0], pixel_type, compression)
    assert ctx.exr() == before                                     # the debug entry point leaves the context's settings alone


# ---------------------------------------------------------------- 2. end to end on a context
def test_float_mean_is_fetch_hdr_over_spp(ctx):
    r = ctx
    r.set_exr(pixel_type="float")
    try:
        assert r.exr() == dict(source="mean", pixel_type="float", compression="zip", chunk_bytes=xr.DEFAULT_CHUNK, scale=1.0, size=(W, H),
                               capacity=xr.capacity(W, H, "float", "zip"))
        want = _oriented(r.fetch_hdr() / F(r.current_spp))
        assert want.dtype == F
        got = r.fetch_exr()
        assert isinstance(got, bytes)
        back, info = exr.read(got)
        assert back.dtype == F and np.array_equal(_bits(back), _bits(want))
        _same(got, xr.encode(want, "float", "zip"), "fetch_exr against the restatement on fetch_hdr / spp")
        view = r.fetch_exr(copy=False)
        assert isinstance(view, memoryview) and view.readonly
        _same(view, got, "the view")
        del view
        p, n = r.render_to_exr()
        assert p and n and p - n == 16                             # the length stands 16 bytes in front of the file
        r.set_exr(pixel_type="half", compression="zips", scale=0.5, chunk_bytes=2048)
        _same(r.fetch_exr(), xr.encode(want, "half", "zips", 2048, 0.5), "half, ZIPS, scale 0.5")
        r.set_exr(compression="none")
        _same(r.fetch_exr(), xr.encode(want, "half", "none"), "half, NONE")
    finally:
        r.set_exr()


def test_each_stage_decodes_to_its_own_fetch_and_refuses_as_it_does(R):
    r = R.Renderer((W, H), (0, 1, 0), **SCENE)
    r.copy_textures()
    r.accumulate(3)
    stages = (("denoised", lambda on: r.set_denoise(on), r.fetch_denoised_hdr),
              ("history", lambda on: r.set_history(on), lambda: r.fetch_history_hdr()[..., :3]),
              ("bloom", lambda on: r.set_bloom(on), r.fetch_bloom_hdr),
              ("local_exposure", lambda on: r.set_local_exposure(on), r.fetch_local_exposure_hdr))
    for source, switch, fetch in stages:
        r.set_exr(source=source, pixel_type="float")
        with pytest.raises(R.DigitalEarthError) as mine:
            r.fetch_exr()                                          # the stage is off
        with pytest.raises(R.DigitalEarthError) as theirs:
            fetch()
        assert mine.value.code == theirs.value.code == ERR_STATE and str(mine.value) == str(theirs.value), source
        with pytest.raises(R.DigitalEarthError) as lagged:
            r.fetch_exr(lag=1)
        assert lagged.value.code == ERR_STATE and r._ex_in_flight == 0
        switch(True)
        try:
            want = _oriented(np.ascontiguousarray(fetch()))
            back = exr.read(r.fetch_exr())[0]
            assert np.array_equal(_bits(back), _bits(want.astype(F))), source
        finally:
            switch(False)
    r.close()


def test_adaptive_frame_divides_every_tile_by_its_own_count(R):
    AW, AH = 128, 64                                               # the adaptive tests' frame (tests/test_gpu_adaptive.py), whose thresholds spread the counts
    r = R.Renderer((AW, AH), (0, 1, 0), texture_source="synthetic", texture_size=(2048, 1024), seed=11)
    r.set_fov(0.42)
    r.copy_textures()
    for tau in (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01):      # the first threshold that leaves tiles at different counts
        r.reset_framebuffer()
        while r.accumulate_adaptive(tau, 32, min_spp=4, round_spp=4) > 0:
            pass
        counts = np.asarray(r.tile_spp())                          # (W / 8, H / 8)
        if len(np.unique(counts)) > 1:
            break
    assert counts.shape == (AW // 8, AH // 8) and counts.min() >= 4 and len(np.unique(counts)) > 1      # a mixed-count frame
    per_pixel = np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1).astype(F)[..., None]
    want = np.ascontiguousarray((r.fetch_hdr() / per_pixel)[:, ::-1].transpose(1, 0, 2))
    r.set_exr(pixel_type="float")
    back = exr.read(r.fetch_exr())[0]
    assert back.shape == (AH, AW, 3) and np.array_equal(_bits(back), _bits(want))
    r.close()


@pytest.mark.parametrize("lag", (1, 2, 3))
def test_ring_hands_out_the_synchronous_bytes(R, lag):
    sync, r = (R.Renderer((W, H), (0, 1, 0), **SCENE) for _ in range(2))      # the same frames twice: one fetched synchronously, one through the ring
    want, got = [], []
    for x in (sync, r):
        x.copy_textures()
        x.set_exr(chunk_bytes=4096)
    for k in range(5):
        sync.accumulate(1); r.accumulate(1)                        # the frames differ by one accumulate
        want.append(sync.fetch_exr())
        out = r.fetch_exr(lag=lag)
        assert (out is None) == (k < lag)
        if out is not None:
            got.append(out)
    with pytest.raises(RuntimeError):
        r.fetch_exr()                                              # a synchronous fetch while lagged ones are in flight
    got += r.fetch_pending_exr(all_images=True)
    assert len(got) == 5 and len({bytes(g) for g in got}) == 5
    for k in range(5):
        _same(got[k], want[k], "lag %d frame %d" % (lag, k))
    assert r.fetch_pending_exr() is None
    sync.close(); r.close()


def test_ring_refusals_and_every_error_code(R, ctx):
    r = ctx
    L, h = r._lib, r._h
    r.set_exr()
    before = r.exr()
    for kw in (dict(chunk_bytes=1023), dict(chunk_bytes=65536), dict(scale=0.0), dict(scale=float("inf")), dict(scale=float("nan"))):
        with pytest.raises(R.DigitalEarthError) as e:
            r.set_exr(**kw)
        assert e.value.code == ERR_INVALID and r.exr() == before
    s = R.DeExr()
    for fields in ((20, 0, 1, 3, 32768, 1.0), (24, 5, 1, 3, 32768, 1.0), (24, 0, 0, 3, 32768, 1.0), (24, 0, 1, 1, 32768, 1.0), (24, 0, 1, 3, 32768, -2.0)):
        s.struct_bytes, s.source, s.pixel_type, s.compression, s.chunk_bytes, s.scale = fields
        assert L.de_set_exr(h, ctypes.byref(s)) == ERR_INVALID and r.exr() == before
    for bad in (dict(source="image"), dict(pixel_type="double"), dict(compression="piz")):
        with pytest.raises(ValueError):
            r.set_exr(**bad)
    full = r.fetch_exr()
    assert r.fetch_exr(lag=1) is None
    with pytest.raises(R.DigitalEarthError) as e:
        r.set_exr(pixel_type="float")                              # while an EXR fetch is in flight
    assert e.value.code == ERR_STATE and r.exr() == before
    for _ in range(3):
        assert L.de_fetch_exr_begin(h) == 0
        r._ex_in_flight += 1
    assert L.de_fetch_exr_begin(h) == ERR_STATE                    # a fifth
    out = r.fetch_pending_exr(all_images=True)
    assert len(out) == 4
    for o in out:
        _same(o, full, "a lagged fetch of the same frame")
    ptr, n = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    assert L.de_fetch_exr_end(h, ctypes.byref(ptr), ctypes.byref(n)) == ERR_STATE      # an _end without a _begin
    small = ctypes.create_string_buffer(b"\xA5" * 40, 40)
    assert L.de_fetch_exr(h, small, ctypes.c_uint64(40), ctypes.byref(n)) == ERR_INVALID and n.value == len(full) and small.raw == b"\xA5" * 40
    img = np.zeros((4, 4, 3), F)
    s.struct_bytes, s.source, s.pixel_type, s.compression, s.chunk_bytes, s.scale = 24, 0, 1, 3, 32768, 1.0
    big = ctypes.create_string_buffer(4096)
    for w_, h_ in ((0, 4), (4, 0), (-1, 4), (1 << 13, (1 << 12) + 1)):
        assert L.de_debug_exr(h, img.ctypes.data, w_, h_, ctypes.byref(s), big, ctypes.c_uint64(4096), ctypes.byref(n)) == ERR_INVALID
    assert L.de_debug_exr(h, img.ctypes.data, 4, 4, ctypes.byref(s), small, ctypes.c_uint64(40), ctypes.byref(n)) == ERR_INVALID      # too small an `out` ...
    assert n.value == len(xr.encode(img)) and small.raw == b"\xA5" * 40                                                                # ... with the length set
    _same(r.fetch_exr(), full, "after the refusals")


def test_lagged_exr_png_and_jpeg_fetches_alternate_on_one_context(R):
    sync, r = (R.Renderer((W, H), (0, 1, 0), **SCENE) for _ in range(2))      # the same frames twice, as above
    for x in (sync, r):
        x.copy_textures()
        x.set_pixels(3, "round")
        x.set_png(chunk_bytes=4096)
        x.set_exr(pixel_type="float", chunk_bytes=2048)
    want, got = [], ([], [], [])
    for k in range(5):
        sync.accumulate(1); r.accumulate(1)
        want.append((sync.fetch_exr(), sync.fetch_png(), sync.fetch_jpeg()))
        order = ((0, r.fetch_exr, 2), (1, r.fetch_png, 1), (2, r.fetch_jpeg, 3))
        for i, fetch, lag in (order if k % 2 == 0 else order[::-1]):      # three rings in flight at once, begun in alternating order
            out = fetch(lag=lag)
            if out is not None:
                got[i].append(out)
    for i, pending in enumerate((r.fetch_pending_exr, r.fetch_pending_png, r.fetch_pending_jpeg)):
        got[i].extend(pending(all_images=True))
    for i in range(3):
        assert len(got[i]) == 5
        for k in range(5):
            _same(got[i][k], want[k][i], "output %d frame %d" % (i, k))
    sync.close(); r.close()


# ---------------------------------------------------------------- 3. nothing moved
@pytest.mark.parametrize("source", ("mean", "bloom"))
def test_other_fetches_are_untouched(R, source):
    r = R.Renderer((W, H), (0, 1, 0), **SCENE)
    r.copy_textures()
    r.accumulate(2)
    r.set_pixels(3, "round")
    r.set_png()
    if source == "bloom":
        r.set_bloom(True)

    def others():
        return r.fetch_image().view(np.uint32).copy(), r.fetch_pixels().copy(), np.frombuffer(r.fetch_png(), np.uint8), r.fetch_hdr().view(np.uint32).copy()
    before = others()
    r.set_exr(source=source)
    first = r.fetch_exr()
    assert r.fetch_exr(lag=1) is None and r.fetch_exr(lag=1) == first
    during = others()
    _same(r.fetch_pending_exr(), first, "the ring beside the other fetches")
    _same(r.fetch_exr(), first, "again")
    for a, b, c in zip(before, during, others()):
        assert (a == b).all() and (a == c).all()
    r.close()


# ---------------------------------------------------------------- 4. the viewer
def test_earth_viewer_frames_saves_and_records(tmp_path):
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(W, H), seed=5, **SCENE)
    v = EarthViewer(**kw)
    path = str(tmp_path / "x.exr")
    v.render(2)
    v.save(path)                                                   # never set: the defaults
    back, info = exr.read(open(path, "rb").read())
    assert back.dtype == np.float16 and back.shape == (H, W, 3) and info["compression"] == "zip"
    want = xr.convert(_oriented(v.renderer.fetch_hdr() / F(v.renderer.current_spp)), 1.0, "half")
    assert np.array_equal(_bits(back), _bits(want))
    v.renderer.set_exr(pixel_type="float", compression="zips")
    v.save(path)
    assert exr.read(open(path, "rb").read())[1]["pixel_type"] == "float"
    for bad in (dict(pixels=True), dict(hdr_pixels=True), dict(video=True), dict(jpeg=True), dict(png=True)):
        with pytest.raises(ValueError):
            v.frame(spp=1, exr=True, **bad)
    v.renderer.reset_framebuffer()
    got = [v.frame(spp=1, exr=True) for k in range(2)]
    assert all(isinstance(g, bytes) for g in got) and got[0] != got[1] and exr.read(got[1])[0].shape == (H, W, 3)
    v.close()
    a, b = EarthViewer(**kw), EarthViewer(**kw)                    # one records, one shows the same frames
    pattern = str(tmp_path / "f%05d.exr")
    angles = [0.2, 0.4, 0.6]
    assert a.record(pattern, 3, sun_angle=angles) == 3
    for k in range(3):
        want = b.frame(spp=1, exr=True, sun_angle=angles[k])
        _same(open(pattern % k, "rb").read(), want, "recorded frame %d" % k)
    with pytest.raises(ValueError):
        a.record(str(tmp_path / "one.exr"), 2)
    assert a.finish_exr() is None
    a.close(); b.close()
