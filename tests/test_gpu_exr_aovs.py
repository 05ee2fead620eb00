"""The EXR output's AOV channels (include/digital_earth_exr_aovs.h) on the GPU: the file of de_debug_exr_aovs equals the numpy
restatement (tests/exr_aov_ref.py) byte for byte on the smallest shapes at which the layout can go wrong; a context's frame decodes to exactly
fetch_guides(), the counts and the variance restated from fetch_hdr() and S2, beside the B, G, R planes of the mask-0 file; the ring hands out the
synchronous fetch's bytes; every refusal answers its code; mask 0 is the three-channel file again."""
import ctypes
import functools

import numpy as np
import pytest

import exr_aov_ref as xa
import exr_ref as xr
from digital_earth_amd import exr

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = -1, -4
W, H = 64, 32
SCENE = dict(texture_source="synthetic", texture_size=(1024, 512))
# 1x1; a row tail that is no multiple of 4; two ZIP blocks, the last of one line; a second workgroup along the row whose last group holds one pixel, on
# the scalar path (1029 = 4 * 257 + 1); the same on the vector path (1032 = 4 * 258)
SHAPES = [(1, 1), (5, 3), (37, 17), (1029, 2), (1032, 1)]
MASKS = [1, 2, 4, 8, 16, 32, 64, 127, 3, 0]
TYPES = ["half", "float"]
COMPRESSIONS = ["zip", "zips", "none"]
# 50 cases: every shape with every mask; the pixel type alternates and the compression cycles along a shape's masks, shifted per shape, so that every
# shape, type, compression and bit meets every other at least once
CASES = [(shape, mask, TYPES[(i + k) % 2], COMPRESSIONS[(i + k) % 3]) for k, shape in enumerate(SHAPES) for i, mask in enumerate(MASKS)]


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def ctx(R):
    r = R.Renderer((W, H), (0, 1, 0), **SCENE)
    r.copy_textures()
    yield r
    r.close()


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """Random float32 sums, guides, S2 and counts with NaN, +-inf, negatives, values beyond 65504, half-subnormals in the guide slots, S2 < S1 mean and
    counts of 1, 2 and more.  Made once per shape and never written to."""
    w, h = shape
    rng = np.random.default_rng(w * 1000 + h)
    image = (rng.standard_normal((h, w, 3)) * 40 + 60).astype(F)
    guides = rng.standard_normal((h, w, 9)).astype(F)
    guides[..., 1] = np.abs(guides[..., 1]) * F(3e5)
    counts = rng.choice(np.array([1, 2, 3, 7, 64], F), size=(h, w)).astype(F)
    s2 = (image * image / counts[..., None] * rng.uniform(0.9, 3.0, (h, w, 3))).astype(F)
    specials = np.array([np.nan, np.inf, -np.inf, -1.5, 65504.0, 65520.0, 1e9, -1e9, 3e-6, -5.9e-8, 6.1e-5, 2.98e-8, 0.0, -0.0], F)
    for a in (image, guides, s2):
        flat = a.reshape(-1)
        at = rng.choice(flat.size, size=max(1, flat.size // 5), replace=False)
        flat[at] = rng.choice(specials, size=at.size)
    if w * h >= 3:
        counts.reshape(-1)[:3] = (1, 2, 7)
    for a in (image, guides, s2, counts):
        a.setflags(write=False)
    return image, guides, s2, counts


def _same(got, want, what=""):
    got, want = bytes(got), bytes(want)
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("%s: %d bytes against %d, first difference at %d" % (what, len(got), len(want), first))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _oriented(field):
    """A (W, H, k) field of the library -> (H, W, k) rows top-down, as fetch_pixels orients the picture."""
    return np.ascontiguousarray(np.asarray(field)[:, ::-1].transpose(1, 0, 2))


# ---------------------------------------------------------------- 1. the kernels, byte for byte
@pytest.mark.parametrize("shape,mask,pixel_type,compression", CASES, ids=["%dx%d-m%d-%s-%s" % (s[0], s[1], m, t, c) for s, m, t, c in CASES])
def test_file_equals_the_restatement(ctx, shape, mask, pixel_type, compression):
    image, guides, s2, counts = _inputs(shape)
    if mask == 0:      # the three-channel entry point's bytes; no array beside the image is read
        got = ctx.debug_exr_aovs(image, aovs=0, pixel_type=pixel_type, compression=compression, chunk_bytes=2048, scale=0.5)
        _same(got, ctx.debug_exr(image, pixel_type=pixel_type, compression=compression, chunk_bytes=2048, scale=0.5), "mask 0 against de_debug_exr")
        _same(got, xr.encode(image, pixel_type, compression, 2048, 0.5), "mask 0 against the three-channel restatement")
        return
    need_guides, need_s2, need_counts = bool(mask & 31), bool(mask & 32), bool(mask & 96)      # what the mask does not need is NULL
    args = (guides if need_guides else None, s2 if need_s2 else None, counts if need_counts else None)
    got = ctx.debug_exr_aovs(image, *args, aovs=mask, pixel_type=pixel_type, compression=compression, chunk_bytes=2048, scale=0.5)      # (checks its own sentinel behind `out`)
    _same(got, xa.encode(image, *args, mask=mask, pixel_type=pixel_type, compression=compression, chunk_bytes=2048, scale=0.5), "the file")
    assert len(got) <= xa.capacity(shape[0], shape[1], pixel_type, compression, mask)
    info = exr.read(got)[1]
    assert info["channel_names"] == [n for n, _ in xa.channel_list(mask, pixel_type)]


def test_debug_refuses_a_missing_array_and_an_unknown_bit(ctx, R):
    image, guides, s2, counts = _inputs((5, 3))
    for kw in (dict(aovs=1), dict(aovs=32, counts=counts), dict(aovs=32, s2=s2), dict(aovs=64), dict(aovs=128, guides=guides, s2=s2, counts=counts)):
        with pytest.raises(R.DigitalEarthError) as e:
            ctx.debug_exr_aovs(image, **kw)
        assert e.value.code == ERR_INVALID, kw


# ---------------------------------------------------------------- 2. a frame
@pytest.fixture(scope="module")
def frame(R):
    """64 x 32, synthetic maps, the denoiser on from the reset, 4 spp, the source `mean`."""
    r = R.Renderer((W, H), (0, 1, 0), **SCENE)
    r.copy_textures()
    r.set_denoise(True)
    r.reset_framebuffer()
    r.accumulate(4)
    yield r
    r.close()


def test_frame_decodes_to_the_guides_the_counts_and_the_variance(frame):
    r = frame
    plain = r.fetch_exr()
    r.set_exr(aovs="all")
    try:
        assert r.exr_aovs() == ("depth", "normal", "albedo", "coverage", "transmittance", "variance", "samples")
        got = r.fetch_exr()
        cap = r.exr()["capacity"]
        assert cap == xa.capacity(W, H, "half", "zip", 127) and len(got) <= cap
        back, info = exr.read(got)
        ch = info["channels"]
        assert info["channel_names"] == [n for n, _ in xa.channel_list(127, "half")]
        back0, info0 = exr.read(plain)
        assert np.array_equal(_bits(back), _bits(back0)) and all(np.array_equal(_bits(ch[n]), _bits(info0["channels"][n])) for n in "BGR")
        guides = _oriented(r.fetch_guides())
        for name, k in (("coverage", 0), ("N.X", 2), ("N.Y", 3), ("N.Z", 4), ("albedo.R", 5), ("albedo.G", 6), ("albedo.B", 7), ("transmittance", 8)):
            assert ch[name].dtype == np.float16 and np.array_equal(_bits(ch[name]), _bits(xr.convert(guides[..., k], 1.0, "half"))), name
        assert ch["Z"].dtype == F and np.array_equal(_bits(ch["Z"]), _bits(xa.float_sample(guides[..., 1])))
        assert (guides[..., 1] > 65504.0).any() and (ch["Z"] > 65504.0).any()          # metres: what a HALF would have clamped
        assert r.current_spp == 4 and ch["samples"].dtype == F and (ch["samples"] == F(4.0)).all()
        s1, s2 = _oriented(r.fetch_hdr()), _oriented(r.adaptive_moments())
        want = xa.variance_of_mean(s1, s2, np.full((H, W), 4.0, F))
        assert want.any()
        for k, name in enumerate(("variance.R", "variance.G", "variance.B")):
            assert ch[name].dtype == F and np.array_equal(_bits(ch[name]), _bits(want[..., k])), name
        _same(got, xa.encode(s1, guides, s2, np.full((H, W), 4.0, F), 127, "half", "zip"), "the frame against the restatement")
        # float, ZIPS, a scale (the radiance's alone), a subset
        r.set_exr(pixel_type="float", compression="zips", scale=0.25, aovs=("normal", "samples"))
        assert r.exr_aovs() == ("normal", "samples")
        _same(r.fetch_exr(), xa.encode(s1, guides, None, np.full((H, W), 4.0, F), 2 | 64, "float", "zips", scale=0.25), "float, ZIPS, normal | samples")
    finally:
        r.set_exr()
    assert r.exr_aovs() == ()
    _same(r.fetch_exr(), plain, "after set_exr(aovs=()) the three-channel file again")


def test_adaptive_frame_holds_samples_and_variance_to_the_tile_counts(R):
    r = R.Renderer((W, H), (0, 1, 0), **SCENE)
    try:
        r.copy_textures()
        r.render_adaptive(0.05, 24, min_spp=8, round_spp=8)
        tiles = np.asarray(r.tile_spp())
        r.set_exr(aovs=("variance", "samples"))
        info = exr.read(r.fetch_exr())[1]
        s1, s2 = _oriented(r.fetch_hdr()), _oriented(r.adaptive_moments())
        n = info["channels"]["samples"]
        assert n.min() >= 8 and n.max() <= 24 and sorted(np.unique(n).tolist()) == sorted(np.unique(tiles).astype(F).tolist())
        assert all(len(np.unique(n[y:y + 8, x:x + 8])) == 1 for y in range(0, H, 8) for x in range(0, W, 8))
        want = xa.variance_of_mean(s1, s2, n)
        for k, name in enumerate(("variance.R", "variance.G", "variance.B")):
            assert np.array_equal(_bits(info["channels"][name]), _bits(want[..., k])), name
        with np.errstate(all="ignore"):
            assert np.array_equal(_bits(exr.read(r.fetch_exr())[0]), _bits(xr.convert((s1 / n[..., None]).astype(F), 1.0, "half")))
    finally:
        r.close()


def test_lagged_fetches_return_the_synchronous_bytes(frame):
    r = frame
    r.set_exr(aovs="all")
    try:
        want = r.fetch_exr()
        got = [r.fetch_exr(lag=2) for _ in range(3)]
        assert got[0] is None and got[1] is None
        rest = r.fetch_pending_exr(all_images=True)
        files = [got[2]] + list(rest)
        assert len(files) == 3
        for f in files:
            _same(f, want, "a lagged fetch")
    finally:
        r.set_exr()


def test_refusals(R):
    r = R.Renderer((W, H), (0, 1, 0), **SCENE)
    try:
        r.copy_textures()
        r.accumulate(2)                                            # no denoiser, no adaptive frame: S2 is incomplete
        r.set_exr(aovs=("variance",))
        for call in (r.fetch_exr, lambda: r.fetch_exr(lag=1), r.render_to_exr):
            with pytest.raises(R.DigitalEarthError) as e:
                call()
            assert e.value.code == ERR_STATE and "denoiser" in str(e.value) and "adaptive" in str(e.value)
        assert r._ex_in_flight == 0
        r.set_denoise(True)                                        # mid-frame: the samples so far have no S2
        with pytest.raises(R.DigitalEarthError) as e:
            r.fetch_exr()
        assert e.value.code == ERR_STATE
        r.set_denoise(False)
        r.set_exr(aovs=("samples", "depth"))                       # these need no S2
        assert (exr.read(r.fetch_exr())[1]["channels"]["samples"] == F(2.0)).all()
        with pytest.raises(ValueError):
            r.set_exr(aovs=("normals",))
        assert r._lib.de_set_exr_aovs(r._h, 128) == ERR_INVALID and r.exr_aovs() == ("depth", "samples")      # a refused call changes nothing
        assert r.fetch_exr(lag=1) is None                          # one fetch in flight
        assert r._lib.de_set_exr_aovs(r._h, 1) == ERR_STATE
        with pytest.raises(R.DigitalEarthError) as e:
            r.set_exr(aovs="all")
        assert e.value.code == ERR_STATE and r.exr_aovs() == ("depth", "samples")
        assert r.fetch_pending_exr() is not None
        r.set_exr()
        fresh = R.Renderer((W, H), (0, 1, 0), **SCENE)
        try:
            fresh.copy_textures()
            fresh.accumulate(2)
            _same(r.fetch_exr(), fresh.fetch_exr(), "after set_exr(aovs=()): the bytes of a fresh renderer")
            assert r.exr() == fresh.exr()
        finally:
            fresh.close()
    finally:
        r.close()


def test_variance_is_refused_where_the_sums_or_s2_are_not_the_frame_s_own(R):
    """As the denoiser, S2's other reader, is (tests/test_gpu_denoise.py): a display source — de_set_display_source leaves S2 marked complete —, a
    sample partition, a tile partition.  The denoiser is on since the reset, so nothing else refuses.  The other groups stay."""
    r = R.Renderer((W, H), (0, 1, 0), **SCENE)
    try:
        r.copy_textures()
        r.set_denoise(True)
        r.reset_framebuffer()
        r.accumulate(2)
        r.set_exr(aovs=("variance", "samples"))
        good = r.fetch_exr()
        L, h = r._lib, r._h
        ptr, n = ctypes.c_void_p(), ctypes.c_uint64()
        assert L.de_hdr_device_ptr(h, ctypes.byref(ptr), ctypes.byref(n)) == 0

        def refused(word):
            for call in (r.fetch_exr, lambda: r.fetch_exr(lag=1), r.render_to_exr):
                with pytest.raises(R.DigitalEarthError) as e:
                    call()
                assert e.value.code == ERR_STATE and word in str(e.value), (word, str(e.value))
            assert r._ex_in_flight == 0
        assert L.de_set_display_source(h, ptr) == 0
        refused("display source")
        r.set_exr(aovs=("samples", "normal"))                      # only the variance group is refused
        assert (exr.read(r.fetch_exr())[1]["channels"]["samples"] == F(2.0)).all()
        r.set_exr(aovs=("variance", "samples"))
        assert L.de_set_display_source(h, None) == 0
        _same(r.fetch_exr(), good, "the display source gone: the file again")
        assert L.de_set_sample_partition(h, 0, 2) == 0
        refused("sample partition")
        assert L.de_set_sample_partition(h, 0, 1) == 0
        _same(r.fetch_exr(), good, "the sample partition gone: the file again")
        assert L.de_accumulate(h, 1, ctypes.c_uint64(0), 0, 2) == 0      # a tile partition
        refused("tile partition")
    finally:
        r.close()


def test_earth_viewer_passes_its_aovs_on(tmp_path):
    from digital_earth_amd.earth_viewer import EarthViewer
    v = EarthViewer(screen_res=(W, H), exr_aovs=("depth",), **SCENE)
    try:
        assert v.renderer.exr_aovs() == ("depth",)
        info = exr.read(v.frame(exr=True))[1]
        assert info["channel_names"] == ["B", "G", "R", "Z"] and info["channel_types"]["Z"] == "float" and (info["width"], info["height"]) == (W, H)
        path = str(tmp_path / "x.exr")
        v.save(path)
        assert exr.read(open(path, "rb").read())[1]["channel_names"] == ["B", "G", "R", "Z"]
        pattern = str(tmp_path / "f%05d.exr")
        v.record(pattern, 2)
        assert all(exr.read(open(pattern % k, "rb").read())[1]["channel_names"] == ["B", "G", "R", "Z"] for k in range(2))
    finally:
        v.close()
