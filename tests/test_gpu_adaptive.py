"""Adaptive sampling (de_accumulate_adaptive): a tile that stopped at n samples holds exactly the bits of a uniform n-spp frame, HDR sums
and displayed image; the sums of squares are the per-sample RGB squared and added in sample order; every decision follows the definition; the limits
(threshold 0, a black scene, the pipelined fetch); nothing of an adaptive frame survives de_reset; every refused call answers its code."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
TAUS = (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01)


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


def _renderer(R, W, H, view="default", seed=11, **kw):
    r = R.Renderer((W, H), (0, 1, 0), texture_source=kw.pop("texture_source", "synthetic"), texture_size=(2048, 1024), seed=seed, **kw)
    if view == "sunset":      # BASELINE cfg4's camera: Earth, limb and space in one view
        from digital_earth_amd.earth_viewer import load_config
        load_config("config - sunset hurricane.txt").apply(r)
    else:
        r.set_fov(0.42)
    r.copy_textures()
    return r


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _pixel_mask(counts, n):
    """(W, H) mask of the pixels whose tile holds n samples; counts = tile_spp() (W/8, H/8)."""
    return np.repeat(np.repeat(counts == n, 8, axis=0), 8, axis=1)


def _adaptive(r, tau, max_spp=32, min_spp=4, round_spp=4, floor=None):
    r.reset_framebuffer()
    kw = {} if floor is None else {"floor": floor}
    info = r.render_adaptive(tau, max_spp, min_spp=min_spp, round_spp=round_spp, **kw)
    return r.tile_spp(), r.fetch_hdr(), r.fetch_image(), info


def _uniform(r, n):
    r.reset_framebuffer()
    r.accumulate(n)
    return r.fetch_hdr(), r.fetch_image()


def _spread_frame(r, max_spp, min_spp, round_spp):
    """The first threshold of TAUS whose frame leaves at least three distinct tile counts, some at max_spp and some below it."""
    for tau in TAUS:
        counts, hdr, img, info = _adaptive(r, tau, max_spp, min_spp, round_spp)
        values = np.unique(counts)
        if len(values) >= 3 and values[-1] == max_spp and values[0] < max_spp:
            return tau, counts, hdr, img, info
    pytest.fail("no threshold of %s spreads the tile counts" % (TAUS,))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("size", [(128, 64), (256, 128)])
@pytest.mark.parametrize("view", ["default", "sunset"])
@pytest.mark.parametrize("variant", [4, 6, 2])
def test_adaptive_tiles_equal_uniform_frames_at_their_count(R, size, view, variant):
    """The core property: for every count n the adaptive frame left, the tiles with n samples equal a uniform n-spp frame of the same seed, bit for
    bit, in fetch_hdr and in fetch_image — whatever kernel renders the rounds."""
    r = _renderer(R, *size, view=view)
    r.set_kernel_variant(variant)
    tau, counts, hdr, img, info = _spread_frame(r, 32, 4, 4)
    assert counts.shape == (size[0] // 8, size[1] // 8) and counts.dtype == np.int32
    assert info["pixel_samples"] == 64 * int(counts.sum())
    assert r.current_spp == int(counts.max()) == 32
    for n in np.unique(counts):
        u_hdr, u_img = _uniform(r, int(n))
        m = _pixel_mask(counts, n)
        assert (_bits(hdr)[m] == _bits(u_hdr)[m]).all(), (tau, n)
        assert (_bits(img)[m] == _bits(u_img)[m]).all(), (tau, n)
    r.close()


@pytest.mark.timeout(600)
def test_adaptive_last_round_clamped_to_max_spp(R):
    """max_spp not a multiple of round_spp: the last round is clamped, no tile passes max_spp, and the equivalence holds at every count."""
    r = _renderer(R, 128, 64, view="sunset")
    tau, counts, hdr, img, info = _spread_frame(r, 30, 4, 8)
    assert counts.max() == 30 and set(np.unique(counts)) <= {8, 16, 24, 30}
    for n in np.unique(counts):
        u_hdr, u_img = _uniform(r, int(n))
        m = _pixel_mask(counts, n)
        assert (_bits(hdr)[m] == _bits(u_hdr)[m]).all() and (_bits(img)[m] == _bits(u_img)[m]).all(), n
    r.close()


@pytest.mark.timeout(600)
def test_moments_are_the_squares_of_every_sample_in_sample_order(R):
    """S2 = sum over s of rgb_s^2 in sample order, f32, no fused multiply-add: each sample's own RGB taken from a fresh one-sample frame at index s."""
    N = 8
    r = _renderer(R, 128, 64, view="sunset")
    r.reset_framebuffer()
    assert r.render_adaptive(0.0, N, min_spp=2, round_spp=3)["rounds"] == 3
    s1, s2 = r.fetch_hdr(), r.adaptive_moments()
    acc1 = np.zeros_like(s1)
    acc2 = np.zeros_like(s1)
    for s in range(N):
        r.reset_framebuffer()
        r.set_current_spp(s)
        r.accumulate(1)
        x = r.fetch_hdr()
        acc1 = acc1 + x
        acc2 = acc2 + x * x
    assert acc2.dtype == np.float32 and acc2.max() > 0
    assert (_bits(acc1) == _bits(s1)).all()
    assert (_bits(acc2) == _bits(s2)).all()
    r.close()


def _decisions(s1, s2, n, tau, floor):
    """Per tile (W/8, H/8), in float64: stays (some pixel and channel has var > tau^2 n (Y^2 + floor^2)) and the deciding relative margin."""
    s1 = s1.astype(np.float64)
    s2 = s2.astype(np.float64)
    mean = s1 / n
    var = np.maximum(0.0, (s2 - s1 * mean) / (n - 1))
    Y = 0.2126 * mean[..., 0] + 0.7152 * mean[..., 1] + 0.0722 * mean[..., 2]
    lim = (tau * tau * n * (Y * Y + floor * floor))[..., None]
    rel = (var - lim) / np.maximum(np.abs(lim), 1e-30)
    W, H = s1.shape[:2]
    per_tile = rel.reshape(W // 8, 8, H // 8, 8, 3).max(axis=(1, 3, 4))
    return per_tile > 0, np.abs(per_tile)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("view", ["default", "sunset"])
def test_every_decision_follows_the_definition(R, view):
    """After every round: a tile that left before max_spp was converged at its count, a tile that was kept was not (margins within 1e-4 exempt)."""
    r = _renderer(R, 256, 128, view=view)
    tau, counts, _, _, _ = _spread_frame(r, 32, 4, 4)
    floor = R.ADAPTIVE_FLOOR
    r.reset_framebuffer()
    snaps = []
    while True:
        active = r.accumulate_adaptive(tau, 32, min_spp=4, round_spp=4)
        snaps.append((r.tile_spp(), r.fetch_hdr(), r.adaptive_moments(), active))
        if active == 0:
            break
    assert (snaps[-1][0] == counts).all()
    checked = 0
    for k, (c, s1, s2, active) in enumerate(snaps):
        n = int(c.max())
        nxt = snaps[k + 1][0] if k + 1 < len(snaps) else c
        kept = nxt > c
        assert int(kept.sum()) == active
        was_active = c == n
        assert not (kept & ~was_active).any()
        if n >= 32:
            assert active == 0
            continue
        if n < 4:
            assert (kept == was_active).all()
            continue
        stays, margin = _decisions(s1, s2, n, tau, floor)
        decided = was_active & (margin > 1e-4)
        assert (kept[decided] == stays[decided]).all(), (k, n, int((kept[decided] != stays[decided]).sum()))
        checked += int(decided.sum())
    assert checked > 0
    r.close()


@pytest.mark.timeout(600)
def test_threshold_zero_is_the_uniform_max_spp_frame(R):
    r = _renderer(R, 128, 64, view="sunset")
    counts, hdr, img, info = _adaptive(r, 0.0, 16, 4, 4)
    assert (counts == 16).all() and info["rounds"] == 4 and info["mean_spp"] == 16.0
    u_hdr, u_img = _uniform(r, 16)
    assert (_bits(hdr) == _bits(u_hdr)).all() and (_bits(img) == _bits(u_img)).all()
    r.close()


@pytest.mark.timeout(600)
def test_a_black_view_stops_every_tile_at_min_spp(R):
    """Constant maps (stars 0) and the camera looking away from the Earth and the sun: zero radiance everywhere, every tile stops at min_spp."""
    r = _renderer(R, 128, 64, texture_source="constant")
    r.set_fov(0.2)
    pos = np.array([-15000000.0, 0.0, 15000000.0])
    for d in ([1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [-1, 0, 1]):
        d = np.asarray(d, dtype=np.float64)
        if np.dot(d, pos) <= 0.0:
            continue      # towards the Earth's side
        r.set_look_at(*(pos + d * 1e6))
        if not _uniform(r, 4)[0].any():
            break
    else:
        pytest.fail("no black view found")
    for floor in (R.ADAPTIVE_FLOOR, 0.0):
        counts, hdr, _, info = _adaptive(r, 0.05, 64, 6, 2, floor=floor)
        assert (counts == 6).all() and not hdr.any() and info["rounds"] == 3
    r.close()


@pytest.mark.timeout(600)
def test_pipelined_fetch_inside_an_adaptive_frame(R):
    """fetch_image(lag=1) after every round returns the previous round's image: the same bits as the synchronous fetch of that round."""
    r = _renderer(R, 128, 64, view="sunset")
    tau = _spread_frame(r, 32, 4, 4)[0]
    sync, lagged = [], []
    r.reset_framebuffer()
    while True:
        active = r.accumulate_adaptive(tau, 32, min_spp=4, round_spp=4)
        sync.append(r.fetch_image())
        if active == 0:
            break
    r.reset_framebuffer()
    while True:
        active = r.accumulate_adaptive(tau, 32, min_spp=4, round_spp=4)
        img = r.fetch_image(lag=1)
        if img is not None:
            lagged.append(img)
        if active == 0:
            break
    lagged.append(r.fetch_pending())
    assert len(sync) == len(lagged) >= 3
    for a, b in zip(sync, lagged):
        assert (_bits(a) == _bits(b)).all()
    r.close()


@pytest.mark.timeout(600)
def test_nothing_of_an_adaptive_frame_survives_reset(R):
    """After an adaptive frame and reset_framebuffer(), a uniform frame equals a fresh context's (the cached tile list, the scalar display)."""
    r = _renderer(R, 128, 64, view="sunset")
    _spread_frame(r, 32, 4, 4)
    r.reset_framebuffer()
    assert r.current_spp == 0 and (r.tile_spp() == 0).all()
    r.accumulate(6)
    got = r.fetch_hdr(), r.fetch_image()
    f = _renderer(R, 128, 64, view="sunset")
    f.accumulate(6)
    want = f.fetch_hdr(), f.fetch_image()
    assert (_bits(got[0]) == _bits(want[0])).all() and (_bits(got[1]) == _bits(want[1])).all()
    f.close()
    r.close()


def _code(fn, *a, **kw):
    from digital_earth_amd._native import DigitalEarthError
    with pytest.raises(DigitalEarthError) as e:
        fn(*a, **kw)
    return e.value.code


@pytest.mark.timeout(600)
def test_refused_calls_answer_their_codes(R, tmp_path):
    from digital_earth_amd import _native
    r = _renderer(R, 128, 64)
    W, H = r.image_res
    go = dict(threshold=0.01, max_spp=16, min_spp=4, round_spp=4)
    # settings
    for bad in (dict(min_spp=1), dict(min_spp=8, max_spp=4), dict(round_spp=0), dict(threshold=-0.1), dict(floor=-1.0), dict(threshold=float("nan"))):
        assert _code(r.accumulate_adaptive, **dict(go, **bad)) == ERR_INVALID, bad
    io = _native.DeAdaptive()
    io.struct_bytes = ctypes.sizeof(io) - 8
    io.threshold, io.min_spp, io.max_spp, io.round_spp = 0.05, 4, 16, 4
    assert r._lib.de_accumulate_adaptive(r._h, ctypes.c_uint64(0), ctypes.byref(io)) == ERR_INVALID
    assert _code(r.adaptive_moments) == ERR_STATE                       # no adaptive frame yet
    # frames that de_accumulate / de_upload_hdr started
    r.accumulate(1)
    assert _code(r.accumulate_adaptive, **go) == ERR_STATE
    r.reset_framebuffer()
    r.upload_hdr(np.zeros((W, H, 3), np.float32), 4)
    assert _code(r.accumulate_adaptive, **go) == ERR_STATE
    r.reset_framebuffer()
    # partitions, the ray marcher
    r.set_sample_partition(0, 2)
    assert _code(r.accumulate_adaptive, **go) == ERR_STATE
    r.set_sample_partition(0, 1)
    r.set_tile_partition(0, 2)
    assert _code(r.accumulate_adaptive, **go) == ERR_STATE
    r.set_tile_partition(0, 1)
    r.set_integrator("ray_marcher")
    assert _code(r.accumulate_adaptive, **go) == ERR_STATE
    r.set_integrator("path_tracer")
    # inside an adaptive frame
    assert r.accumulate_adaptive(**go) > 0
    assert _code(r.accumulate, 1) == ERR_STATE
    assert _code(r.upload_hdr, np.zeros((W, H, 3), np.float32), 4) == ERR_STATE
    assert _code(r.set_current_spp, 3) == ERR_STATE
    assert _code(r.reduce) == ERR_STATE
    assert _code(r.reduce_progressive) == ERR_STATE
    assert _code(r.reduce_ordered) == ERR_STATE
    with pytest.raises(RuntimeError):
        r.save_checkpoint(str(tmp_path / "ck.npz"))
    assert _code(r.accumulate_adaptive, **dict(go, threshold=0.02)) == ERR_INVALID
    assert _code(r.accumulate_adaptive, **dict(go, round_spp=2)) == ERR_INVALID
    assert _code(r.accumulate_adaptive, **dict(go, floor=0.5)) == ERR_INVALID
    r.seed += 1
    assert _code(r.accumulate_adaptive, **go) == ERR_INVALID
    r.seed -= 1
    # the refused calls changed nothing: the frame finishes, and a call after that renders nothing and answers the same
    while r.accumulate_adaptive(**go) > 0:
        pass
    before = dict(r._adaptive), r.fetch_hdr(), r.current_spp
    assert r.accumulate_adaptive(**go) == 0
    after = r._adaptive
    assert after["rounds"] == before[0]["rounds"] and after["pixel_samples"] == before[0]["pixel_samples"]
    assert (after["tile_spp"] == before[0]["tile_spp"]).all() and r.current_spp == before[2]
    assert (_bits(r.fetch_hdr()) == _bits(before[1])).all()
    r.close()


@pytest.mark.timeout(600)
def test_viewer_renders_to_noise(R, tmp_path):
    """EarthViewer.render_to_noise / start(noise=...): the adaptive frame behind the headless viewer; noise=None keeps the uniform frame."""
    from digital_earth_amd.earth_viewer import EarthViewer
    v = EarthViewer(screen_res=(128, 64), texture_source="synthetic", texture_size=(2048, 1024), seed=11)
    img = v.render_to_noise(0.05, 32, min_spp=4, round_spp=4)
    assert img.shape == (128, 64, 3) and np.isfinite(img).all()
    assert 4 <= v.last_adaptive["mean_spp"] <= 32 and v.renderer.tile_spp().max() <= 32
    out = v.start(spp=16, out=str(tmp_path / "a.npy"), noise=0.05)
    assert np.load(out).shape == (128, 64, 3) and v.renderer.tile_spp().max() <= 16
    v.renderer.reset_framebuffer()
    v.start(spp=4, out=str(tmp_path / "b.npy"))
    assert v.renderer.current_spp == 4 and (v.renderer.tile_spp() == 4).all()
    v.close()
