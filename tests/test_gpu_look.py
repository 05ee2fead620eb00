"""The look LUTs (include/digital_earth_look.h) on the GPU: look_apply_kernel equals the numpy restatement (tests/look_ref.py) bit for
bit, on arbitrary pixel arrays through de_debug_look and end to end behind the unchanged display transform, where every fetch of the displayed
image delivers the graded image and nothing else changes; the stage off, or on at strength 0, gives the bytes it gave before the stage existed.

Pixel counts: 1 and 3 are tail only (no float4 group); 4 is one group and no tail; 5 one group and a tail; 255 / 256 / 257 the same around a wave
boundary; 1023 is one workgroup with a 3-pixel tail in its last wave; 4100 = 1025 groups: a fifth workgroup with one active thread.
3D edges: 2 and 3 the smallest (every cell at a border), 17 / 33 / 65 the sizes .cube files have (65 the limit: the largest index);
1D sizes: 2, 1024 and the limit 65536."""
import ctypes

import numpy as np
import pytest

import hdr_output_ref as ho
import look_ref as lr
import output_scale_ref as osr
import pixels_ref as px
import video_ref as vr
from digital_earth_amd import cube as cube_mod

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID = -1
COUNTS = (1, 3, 4, 5, 255, 256, 257, 1023, 4100)
SIZES_3D = (2, 3, 17, 33, 65)
SIZES_1D = (2, 1024, 65536)
STRENGTHS = (0.0, 0.37, 1.0)
SPECIAL = np.array([-0.0, np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-45, -1e-45, 1.0, 0.0, 1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, 2.0, -2.0, 0.5], F)
W, H = 48, 24

_TABLES = {}


def table(kind, n, domain="default"):
    """White noise over [-0.25, 1.25]: nothing about a neighbour can be guessed from an entry.  domain "other": a different span on every channel.
    Built once per (kind, size, domain) and never written to."""
    key = (kind, n, domain)
    if key not in _TABLES:
        rng = np.random.default_rng(n + (7 if kind == "1d" else 0) + (100000 if domain == "other" else 0))
        values = rng.uniform(-0.25, 1.25, cube_mod.rows(kind, n) * 3).astype(F)
        lo, hi = ((0.0,) * 3, (1.0,) * 3) if domain == "default" else ((-0.25, 0.0, 0.125), (1.0, 1.5, 0.875))
        _TABLES[key] = cube_mod.Cube(kind, n, values, lo, hi)
    return _TABLES[key]


def grade():
    """A look one could ship: a warm, lifted 17^3 grade with a cross-channel term, values in [0, 1]."""
    if "grade" not in _TABLES:
        a = np.linspace(0.0, 1.0, 17)
        b, g, r = np.meshgrid(a, a, a, indexing="ij")
        T = np.stack([0.04 + 0.9 * r ** 0.8 + 0.05 * g * (1 - b), 0.02 + 0.95 * g ** 1.1 - 0.03 * r * b, 0.9 * b ** 1.3 + 0.08 * (r + g) / 2], -1)
        _TABLES["grade"] = cube_mod.Cube("3d", 17, np.clip(T, 0, 1).astype(F))
    return _TABLES["grade"]


def pixels(n, seed=0):
    """n x 3 inputs over and around [0, 1]: random; from the 16th pixel on also ties of two and three channels and points of the 17-lattice; the
    special values at the odd flat indices, as many as fit."""
    rng = np.random.default_rng(1000 + n + seed)
    x = rng.uniform(-0.2, 1.2, (n, 3)).astype(F)
    if n >= 64:
        k = n // 8
        x[16:16 + k, 1] = x[16:16 + k, 0]                                    # fr == fg
        x[16 + k:16 + 2 * k] = x[16 + k:16 + 2 * k, :1]                      # all equal
        x[16 + 2 * k:16 + 3 * k] = (rng.integers(0, 17, (k, 3)) / 16.0).astype(F)      # lattice points of every edge 2, 3, 5, 9, 17, and cell faces of 33, 65
        x[16 + 3 * k:16 + 4 * k, 2] = (rng.integers(0, 65, k) / 64.0).astype(F)        # one coordinate on a face
    flat = x.reshape(-1)
    m = min(len(SPECIAL), flat.size // 2)
    flat[1:2 * m:2] = SPECIAL[:m]
    x.flags.writeable = False
    return x


CHAINS = ([dict(cube=("3d", n, d)) for n in SIZES_3D for d in ("default", "other")]
          + [dict(shaper=("1d", n, d)) for n in SIZES_1D for d in ("default", "other")]
          + [dict(shaper=("1d", 1024, "default"), cube=("3d", 17, "other")), dict(shaper=("1d", 2, "other"), cube=("3d", 65, "default")),
             dict(shaper=("1d", 65536, "other"), cube=("3d", 2, "other"))])


def _chain(spec):
    return {k: table(*v) for k, v in spec.items()}


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def small(R):
    """One Renderer on 1x1 maps at 48 x 24, shared by the tests that only upload sums and display."""
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    r.copy_textures()
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    a, b = (_bits(got), _bits(want)) if got.dtype == F else (got, want)
    diff = a != b
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def _sums(seed=0):
    """Sums whose display covers black, saturated colours, mid greys and clipped white."""
    rng = np.random.default_rng(100 * W + H + seed)
    s = (np.exp2(rng.uniform(-9.0, 3.0, (W, H, 1))) * rng.uniform(0.3, 1.6, (W, H, 3))).astype(F)
    s[: W // 4, : H // 4] = 0.0
    return s


# ---------------------------------------------------------------- 1. the kernel, bit for bit
@pytest.mark.parametrize("n", COUNTS)
def test_kernel_equals_the_restatement(small, n):
    """Every chain (3D only at five edges, 1D only at three sizes, both; a default and a non-default domain each) x both interpolations x three
    strengths at one pixel count.  A 1D-only chain has no interpolation to vary: it runs once per strength."""
    x = pixels(n)
    before = small.look()
    for spec in CHAINS:
        chain = _chain(spec)
        for interpolation in (lr.INTERPOLATIONS if "cube" in chain else ("tetrahedral",)):
            for s in STRENGTHS:
                got = small.debug_look(x, strength=s, interpolation=interpolation, **chain)
                _same(got, lr.apply(x, strength=s, interpolation=interpolation, **chain), (n, spec, interpolation, s))
    assert small.look() == before                  # the debug entry point leaves the context's look alone


def test_special_values_and_the_exact_properties(small):
    """Each special value in each channel, beside ordinary ones, through every chain; then the header's exact properties on the device itself."""
    n = len(SPECIAL)
    x = np.full((3 * n, 3), 0.4, F)
    for c in range(3):
        x[c * n:(c + 1) * n, c] = SPECIAL
    x = np.concatenate([x, np.repeat(SPECIAL[:, None], 3, 1)])
    for spec in CHAINS:
        chain = _chain(spec)
        for interpolation in (lr.INTERPOLATIONS if "cube" in chain else ("tetrahedral",)):
            for s in STRENGTHS:
                got = small.debug_look(x, strength=s, interpolation=interpolation, **chain)
                _same(got, lr.apply(x, strength=s, interpolation=interpolation, **chain), (spec, interpolation, s))
                assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all() and not np.signbit(got).any()
    unit = np.random.default_rng(4).uniform(0, 1, (1000, 3)).astype(F)
    unit[:3] = ((0, 0, 0), (1, 1, 1), (0, 1, 0.5))
    g = grade()
    T = np.frombuffer(g.table, dtype=F).reshape(17, 17, 17, 3)
    idx = np.random.default_rng(5).integers(0, 17, (1000, 3))
    for interpolation in lr.INTERPOLATIONS:
        _same(small.debug_look(unit, cube=table("3d", 33), strength=0.0, interpolation=interpolation), unit, "strength 0 is the identity on [0, 1]")
        _same(small.debug_look((idx / 16.0).astype(F), cube=g, interpolation=interpolation), T[idx[:, 2], idx[:, 1], idx[:, 0]], "a lattice point is its entry")
        _same(small.debug_look(np.ones((1, 3), F), cube=g, interpolation=interpolation), T[16, 16, 16][None], "1.0 is the last entry")
    _same(small.debug_look(unit, shaper=table("1d", 65536), strength=0.0), unit)
    ident = cube_mod.identity(17)
    _same(small.debug_look((idx / 16.0).astype(F), cube=ident), (idx / 16.0).astype(F), "the identity table at its lattice")


# ---------------------------------------------------------------- 2. through a context
def _device_floats(r, ptr, n):
    """n floats at a device address, copied out by the HIP runtime that the library itself runs on (the one this process has loaded)."""
    r.synchronize()
    with open("/proc/self/maps") as maps:
        path = next(line.split()[-1] for line in maps if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMemcpy.restype, hip.hipMemcpy.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    out = np.empty(n, F)
    assert hip.hipMemcpy(out.ctypes.data, ptr, n * 4, 2) == 0      # hipMemcpyDeviceToHost
    return out


def test_every_fetch_of_the_displayed_image_is_graded(R, small):
    r = small
    sums = _sums()
    never = R.Renderer((W, H), (0, 1, 0), texture_source="constant")      # the feature is never touched on this one
    never.copy_textures()
    never.upload_hdr(sums, 2)
    r.upload_hdr(sums, 2)
    assert r.look() is None
    shown = r.fetch_image()
    hdr = r.fetch_hdr()
    _same(shown, never.fetch_image())
    looks = (dict(cube=grade()), dict(cube=table("3d", 33, "other"), shaper=table("1d", 1024), strength=0.37, interpolation="trilinear"),
             dict(shaper=table("1d", 2, "other"), strength=1.0))
    for kw in looks:
        r.set_look(**kw)
        info = r.look()
        assert info["enabled"] and info["strength"] == F(kw.get("strength", 1.0)) and info["interpolation"] == kw.get("interpolation", "tetrahedral")
        assert info["cube_size"] == (kw["cube"].size if "cube" in kw else 0) and info["shaper_size"] == (kw["shaper"].size if "shaper" in kw else 0)
        graded = lr.apply(shown, **kw)
        assert (_bits(graded) != _bits(shown)).any()
        _same(r.fetch_image(), graded, "fetch_image")
        view = r.fetch_image(copy=False)
        _same(np.array(view), graded, "the view")
        del view
        _same(_device_floats(r, r.render_to_image_device(), W * H * 3).reshape(W, H, 3), graded, "render_to_image_device")
        for channels, mode in ((4, "round"), (3, "dither")):
            r.set_pixels(channels, mode, seed=3)
            _same(r.fetch_pixels(), px.pack(graded, channels, mode, 3, 0), "fetch_pixels")
        r.set_pixels()
        r.set_video("i420", siting="center")
        _same(r.fetch_video(), vr.pack(graded, "i420", siting="center"), "fetch_video")
        r.set_video()
        # the lagged ring: begun under this look, handed out later
        assert r.fetch_image(lag=1) is None
        _same(r.fetch_image(lag=1), graded, "the ring")
        _same(r.fetch_pending(), graded, "the ring's last")
        # behind the stage: output scaling resamples the graded image, and the pack kernels read the resampled one
        r.set_output_scale((32, 16), filter="mitchell")
        tables = (r.debug_output_scale_weights(W, 32, "mitchell"), r.debug_output_scale_weights(H, 16, "mitchell"))
        scaled = osr.resample(graded, (32, 16), "mitchell", tables=tables)
        _same(r.fetch_image(), scaled, "scaled")
        _same(_device_floats(r, r.render_to_image_device(), 32 * 16 * 3).reshape(32, 16, 3), scaled, "render_to_image_device, scaled")
        r.set_pixels(4, "round")
        _same(r.fetch_pixels(), px.pack(scaled, 4, "round"), "scaled pixels")
        r.set_pixels()
        r.set_video("nv12")
        _same(r.fetch_video(), vr.pack(scaled, "nv12"), "scaled video")
        r.set_video()
        r.set_output_scale(on=False)
        _same(r.fetch_hdr(), hdr, "fetch_hdr")                  # the sums are not the stage's business
    # the HDR signal: the stage grades whatever the display wrote
    r.set_look(enabled=False)
    assert r.look() is None
    _same(r.fetch_image(), shown, "off again")
    r.set_hdr_output(True, peak_nits=1000.0, gamut="rec709", transfer="pq", pixel_format="rgb16", mode="round")
    signal = r.fetch_image()
    assert (_bits(signal) != _bits(shown)).any()
    r.set_look(cube=grade(), strength=0.37)
    graded = lr.apply(signal, cube=grade(), strength=0.37)
    _same(r.fetch_image(), graded, "the HDR signal")
    _same(r.fetch_hdr_pixels(), ho.pack(graded, "rgb16", "round"), "fetch_hdr_pixels")
    r.set_hdr_output(True, peak_nits=1000.0, gamut="rec709", transfer="pq", pixel_format="rgb10a2", mode="truncate")
    _same(r.fetch_hdr_pixels(), ho.pack(graded, "rgb10a2", "truncate"), "fetch_hdr_pixels, 10 bits")
    r.set_hdr_output(False)
    r.set_look(enabled=False)
    _same(r.fetch_image(), shown, "off at the end")
    _same(never.fetch_image(), shown)
    never.close()


def test_intermediate_fetches_do_not_change(R):
    """Two contexts through the same calls, one with the look on: the sums and every intermediate mean are equal; only the image differs."""
    pair = [R.Renderer((W, H), (0, 1, 0), texture_source="constant") for _ in range(2)]
    for r in pair:
        r.copy_textures()
        r.set_denoise(True)
        r.set_history(True)
        r.set_bloom(True, intensity=0.3)
        r.set_local_exposure(True)
    pair[0].set_look(cube=grade())
    for frame in range(2):
        got = []
        for r in pair:
            r.upload_hdr(_sums(frame), 2)
            one = [r.fetch_image(), r.fetch_hdr(), r.fetch_denoised_hdr(), r.fetch_history_hdr(), r.fetch_bloom_hdr(), r.fetch_local_exposure_hdr(), r.fetch_image()]
            got.append([np.asarray(p) for part in one for p in (part if isinstance(part, (tuple, list)) else (part,))])
        assert len(got[0]) == len(got[1]) >= 7
        for k in range(1, len(got[0]) - 1):
            _same(got[0][k], got[1][k], ("intermediate", frame, k))
        for k in (0, len(got[0]) - 1):
            _same(got[0][k], lr.apply(got[1][k], cube=grade()), ("image", frame, k))
    for r in pair:
        r.close()


def test_off_strength_0_and_the_identity_table(small):
    r = small
    r.upload_hdr(_sums(2), 2)
    r.set_look(enabled=False)
    today = r.fetch_image()
    r.set_pixels(4, "truncate")
    today_px = r.fetch_pixels()
    # on at strength 0: today's bytes, whatever the table
    r.set_look(cube=table("3d", 17), shaper=table("1d", 1024, "other"), strength=0.0)
    assert r.look()["strength"] == 0.0
    _same(r.fetch_image(), today, "strength 0")
    _same(r.fetch_pixels(), today_px, "strength 0, pixels")
    # off: today's bytes
    r.set_look(enabled=False)
    _same(r.fetch_image(), today, "off")
    _same(r.fetch_pixels(), today_px, "off, pixels")
    r.set_pixels()
    # an identity table over a lattice-aligned image (a display source of k / 16, shown as it is by neither route: the restatement decides)
    r.set_look(cube=cube_mod.identity(17))
    _same(r.fetch_image(), lr.apply(today, cube=cube_mod.identity(17)), "identity table")
    aligned = (np.random.default_rng(6).integers(0, 17, (1, W * H, 3)) / 16.0).astype(F)
    _same(r.debug_look(aligned, cube=cube_mod.identity(17)), aligned, "identity table at its lattice")
    _same(lr.apply(aligned, cube=cube_mod.identity(17)), aligned)
    # set_look() without tables keeps the ones held
    r.set_look(enabled=False)
    r.set_look(strength=0.5)
    assert r.look()["cube_size"] == 17 and r.look()["strength"] == 0.5
    _same(r.fetch_image(), lr.apply(today, cube=cube_mod.identity(17), strength=0.5))
    r.set_look(enabled=False)


def test_refusals_leave_the_previous_look_in_force(R, small):
    from digital_earth_amd import _native
    r = small
    L, h = r._lib, r._h
    r.upload_hdr(_sums(3), 2)
    r.set_look(enabled=False)
    plain = r.fetch_image()
    r.set_look(cube=grade(), shaper=table("1d", 2, "other"), strength=0.75, interpolation="trilinear")
    held = r.look()
    want = lr.apply(plain, cube=grade(), shaper=table("1d", 2, "other"), strength=0.75, interpolation="trilinear")
    _same(r.fetch_image(), want)
    t1 = np.linspace(0, 1, 12, dtype=F)
    t3 = np.linspace(0, 1, 24, dtype=F)

    def settings(**kw):
        s = _native.DeLook()
        s.struct_bytes, s.enabled, s.interpolation, s.strength, s.size_1d, s.size_3d = ctypes.sizeof(s), 1, 1, 1.0, 4, 2
        for name in ("max_1d", "max_3d"):
            setattr(s, name, (ctypes.c_float * 3)(1.0, 1.0, 1.0))
        for k, v in kw.items():
            setattr(s, k, (ctypes.c_float * 3)(*v) if isinstance(v, tuple) else v)
        return s
    assert L.de_set_look(h, ctypes.byref(settings(enabled=0)), t1.ctypes.data, t3.ctypes.data) == 0      # the settings are good ones ...
    assert r.look() is None
    r.set_look(cube=grade(), shaper=table("1d", 2, "other"), strength=0.75, interpolation="trilinear")
    nan, inf = float("nan"), float("inf")
    bad = [dict(struct_bytes=68), dict(struct_bytes=76), dict(interpolation=-1), dict(interpolation=2), dict(strength=-0.01), dict(strength=1.01), dict(strength=nan),
           dict(size_1d=1), dict(size_1d=-1), dict(size_1d=65537), dict(size_3d=1), dict(size_3d=-2), dict(size_3d=66), dict(size_1d=0, size_3d=0),
           dict(max_1d=(1.0, 0.0, 1.0)), dict(min_3d=(0.0, 1.0, 0.0)), dict(max_3d=(1.0, inf, 1.0)), dict(min_1d=(nan, 0.0, 0.0)), dict(min_3d=(-inf, 0.0, 0.0)),
           dict(min_1d=(0.0, 0.0, 0.0), max_1d=(1e-45, 1.0, 1.0))]
    for kw in bad:                                                                                           # ... until one thing is wrong
        assert L.de_set_look(h, ctypes.byref(settings(**kw)), t1.ctypes.data, t3.ctypes.data) == ERR_INVALID, kw
        assert r.look() == held, kw
    assert L.de_set_look(h, ctypes.byref(settings()), None, t3.ctypes.data) == ERR_INVALID                   # a null table for a non-zero size
    assert L.de_set_look(h, ctypes.byref(settings()), t1.ctypes.data, None) == ERR_INVALID
    assert L.de_set_look(h, ctypes.byref(settings(size_1d=0)), None, t3.ctypes.data) == 0                    # a null table of size 0 is no table
    r.set_look(cube=grade(), shaper=table("1d", 2, "other"), strength=0.75, interpolation="trilinear")
    for value in (nan, inf, -inf):
        for which in (0, 1):
            a, b = t1.copy(), t3.copy()
            (a, b)[which][5] = value
            assert L.de_set_look(h, ctypes.byref(settings()), a.ctypes.data, b.ctypes.data) == ERR_INVALID, (value, which)
    assert L.de_set_look(h, None, t1.ctypes.data, t3.ctypes.data) == ERR_INVALID and L.de_set_look(None, ctypes.byref(settings()), t1.ctypes.data, t3.ctypes.data) == ERR_INVALID
    assert L.de_get_look(h, None) == ERR_INVALID
    assert r.look() == held
    _same(r.fetch_image(), want, "the previous look is still in force")
    out = np.empty((4, 3), F)
    x = np.zeros((4, 3), F)
    assert L.de_debug_look(h, x.ctypes.data, ctypes.c_uint64(4), ctypes.byref(settings()), t1.ctypes.data, t3.ctypes.data, out.ctypes.data) == 0
    assert L.de_debug_look(h, x.ctypes.data, ctypes.c_uint64(0), ctypes.byref(settings()), t1.ctypes.data, t3.ctypes.data, out.ctypes.data) == ERR_INVALID
    assert L.de_debug_look(h, x.ctypes.data, ctypes.c_uint64(4), ctypes.byref(settings(size_1d=0, size_3d=0, enabled=0)), None, None, out.ctypes.data) == ERR_INVALID
    assert L.de_debug_look(h, x.ctypes.data, ctypes.c_uint64(4), ctypes.byref(settings(strength=2.0)), t1.ctypes.data, t3.ctypes.data, out.ctypes.data) == ERR_INVALID
    assert L.de_debug_look(h, None, ctypes.c_uint64(4), ctypes.byref(settings()), t1.ctypes.data, t3.ctypes.data, out.ctypes.data) == ERR_INVALID
    for kw in (dict(interpolation="cubic"), dict(cube=table("1d", 2)), dict(shaper=grade())):
        with pytest.raises(ValueError):
            r.set_look(**kw)
    assert r.look() == held
    r.set_look(enabled=False)


def test_a_new_look_takes_effect_on_the_same_frame(small):
    """No de_reset, no new samples: the display runs again at every fetch and the stage works on what it wrote.  Lagged fetches may be in flight while
    the look changes: each hands out the look it was begun under."""
    r = small
    r.upload_hdr(_sums(4), 2)
    r.set_look(enabled=False)
    plain = r.fetch_image()
    a, b = dict(cube=grade()), dict(cube=table("3d", 65), strength=0.37, interpolation="trilinear")
    r.set_look(**a)
    _same(r.fetch_image(), lr.apply(plain, **a))
    r.set_look(**b)
    _same(r.fetch_image(), lr.apply(plain, **b))
    r.set_look(**a)
    assert r.fetch_image(lag=2) is None                  # begun under a
    r.set_look(**b)
    assert r.fetch_image(lag=2) is None                  # begun under b
    r.set_look(enabled=False)
    _same(r.fetch_image(lag=2), lr.apply(plain, **a), "begun under the first look")
    rest = r.fetch_pending(all_images=True)
    assert len(rest) == 2
    _same(rest[0], lr.apply(plain, **b), "begun under the second")
    _same(rest[1], plain, "begun with the stage off")
    _same(r.fetch_image(), plain)


def test_earth_viewer_takes_a_look(tmp_path):
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(64, 32), texture_source="synthetic", texture_size=(1024, 512), seed=5)
    path = str(tmp_path / "grade.cube")
    cube_mod.write_cube(path, grade())
    plain, graded = EarthViewer(**kw), EarthViewer(look=path, look_strength=0.5, **kw)
    assert graded.renderer.look()["cube_size"] == 17 and graded.renderer.look()["strength"] == 0.5 and plain.renderer.look() is None
    for k in range(2):
        _same(graded.frame(spp=1), lr.apply(plain.frame(spp=1).copy(), cube=grade(), strength=0.5), k)
    plain.close()
    graded.close()
