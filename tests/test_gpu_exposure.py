"""Auto-exposure (include/digital_earth_exposure.h) on the GPU: the histogram equals the numpy restatement (tests/exposure_f64.py) exactly on
synthetic sums; the EV agrees with the float64 restatement within 2 ulp of f32; the adaptation recurrence; the display is the unchanged transform at
the metered EV, bit for bit, from every source the display reads; the pipelined window loop; every error answers its code.

Sizes: 16x8 is one partial workgroup, 80x40 has partial 32x32 display blocks and a pixel count that is no multiple of the meter's stride, 64x32 is the
default small size."""
import ctypes

import numpy as np
import pytest

import exposure_f64 as ae

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
SIZES = [(16, 8), (80, 40), (64, 32)]
SPPS = (1, 7)
TAUS = (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01)
# the defaults; a tight window with compensation and an EV clamp that bites on the dark images; a strict sub-rectangle aligned to neither 4, 8 nor 32
SETTINGS = {
    "defaults": lambda W, H: dict(),
    "tight": lambda W, H: dict(percentiles=(0.45, 0.55), compensation=0.7, ev_range=(-1.0, 1.5), key=0.25),
    "region": lambda W, H: dict(region=(3, 1, W - 2, H - 1)),
}


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


@pytest.fixture(scope="module")
def contexts(R):
    """One Renderer on 1x1 maps per size, shared by the tests that only upload sums and display."""
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[(W, H)] = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
            made[(W, H)].copy_textures()
        return made[(W, H)]
    yield get
    for r in made.values():
        r.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _edge_values(spp):
    """Green-only sums s whose luminance 0.7152f * (s / spp) lies on a bin edge or within a few ulp of one, for every edge and both range ends: the
    seven neighbouring f32 values around spp * edge / 0.7152f.  Division and product are monotone, so they straddle the edge in steps of about one ulp."""
    w = np.float32(0.7152)
    out = []
    for e in ae.bin_edges().astype(np.float32):
        cand = [np.float32(np.float32(e / w) * np.float32(spp))]
        for _ in range(3):
            cand = [np.nextafter(cand[0], np.float32(0))] + cand + [np.nextafter(cand[-1], np.float32(np.inf))]
        out.extend(cand)
    return np.array(out, np.float32)


_INPUTS = {}


def _inputs(W, H):
    """name -> (W, H, 3) float32 sums, made once per size."""
    if (W, H) in _INPUTS:
        return _INPUTS[(W, H)]
    rng = np.random.default_rng(1000 * W + H)
    n = W * H
    # log-uniform luminances over 2^-30 .. 2^10 with random chroma, negative channels included
    Y = np.exp2(rng.uniform(-30.0, 10.0, n))
    chroma = rng.uniform(-0.6, 2.0, (n, 3))
    mixed = (Y[:, None] * chroma).astype(np.float32)
    k = rng.permutation(n)
    q = max(n // 16, 2)
    mixed[k[:q]] = 0.0                                                     # exact zeros
    mixed[k[q:2 * q]] = -np.abs(mixed[k[q:2 * q]]) - np.float32(1e-3)      # negative luminance
    mixed[k[2 * q:3 * q]] = np.float32(1e-40) * rng.integers(1, 1000, (q, 3)).astype(np.float32)      # subnormals
    # exactly on and next to bin edges; both range ends always present
    n_ev = len(_edge_values(1))
    ends = np.concatenate([np.arange(7), np.arange(n_ev - 7, n_ev)])
    pick = np.concatenate([ends, rng.choice(n_ev, n - len(ends), replace=n - len(ends) > n_ev)])[rng.permutation(n)]
    edges = {}
    for spp in SPPS:                                                       # the same edges at every count: the sums are scaled by it
        edges[spp] = np.zeros((n, 3), np.float32)
        edges[spp][:, 1] = _edge_values(spp)[pick]
    constant = np.full((n, 3), 0.4, np.float32)                            # every pixel in one bin: all 64 lanes of every wave on one LDS address
    below = (np.exp2(rng.uniform(-40.0, -25.0, n))[:, None] * np.array([1.0, 1.0, 1.0])).astype(np.float32)
    below[k[:q]] = 0.0
    bright = (np.exp2(rng.uniform(-6.0, 3.0, n))[:, None] * rng.uniform(0.5, 1.5, (n, 3))).astype(np.float32)      # an ordinary scene: no clamp bites
    named = dict(mixed=mixed, constant=constant, below=below, bright=bright)
    named.update({"edges@%d" % spp: e for spp, e in edges.items()})
    _INPUTS[(W, H)] = {name: a.reshape(W, H, 3) for name, a in named.items()}
    return _INPUTS[(W, H)]


def _cases(W, H, spp):
    """(name, sums) of every input at one sample count: the edge image is the one made for that count."""
    for name, sums in _inputs(W, H).items():
        if "@" not in name:
            yield name, sums
        elif name == "edges@%d" % spp:
            yield "edges", sums


def _show(r, sums, spp):
    r.upload_hdr(sums, spp)
    r.fetch_image()
    return r.metering()


def _same_histogram(m, want):
    assert m["histogram"].dtype == np.uint32 and m["histogram"].shape == (256,)
    assert (m["histogram"] == want["histogram"]).all(), np.nonzero(m["histogram"] != want["histogram"])[0][:8]
    assert (m["metered"], m["below"], m["clipped"]) == (want["metered"], want["below"], want["clipped"])


# ---------------------------------------------------------------- 1. the histogram, exactly
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("size", SIZES)
def test_histogram_equals_the_restatement_exactly(contexts, size, spp):
    W, H = size
    r = contexts(W, H)
    r.set_auto_exposure(True)
    for name, sums in _cases(W, H, spp):
        m = _show(r, sums, spp)
        want = ae.meter(sums, spp)
        _same_histogram(m, want)
        assert m["metered"] + m["below"] == W * H
        if name == "constant":
            assert m["histogram"].max() == W * H
        if name == "below":
            assert m["metered"] == 0 and m["below"] == W * H and not m["valid"]
        if name == "edges":
            assert m["histogram"][0] > 0 and m["clipped"] > 0 and m["below"] > 0      # both range ends were hit from both sides
            with np.errstate(all="ignore"):
                Y = ae.luminance(sums / np.float32(spp)).ravel()
            on_edge = np.isin(Y, ae.bin_edges().astype(np.float32))
            assert on_edge.sum() >= 8 and Y[on_edge].min() == ae.Y_MIN and Y[on_edge].max() == ae.Y_MAX      # luminances exactly on edges, the two ends among them
    r.set_auto_exposure(False)


# ---------------------------------------------------------------- 2. the EV, within 2 ulp of f32
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("size", SIZES)
def test_ev_within_2_ulp_of_the_f64_restatement(contexts, size, setting):
    W, H = size
    r = contexts(W, H)
    kw = SETTINGS[setting](W, H)
    manual = float(r.exposure[None])
    clamped = 0
    for spp in SPPS:
        for name, sums in _cases(W, H, spp):
            r.set_auto_exposure(True, **kw)          # clears the state: every metering is a first one
            got = r.auto_exposure()
            assert got["region"] == kw.get("region") and got["percentiles"] == tuple(float(np.float32(x)) for x in kw.get("percentiles", (0.10, 0.95)))
            m = _show(r, sums, spp)
            want_h = ae.meter(sums, spp, region=kw.get("region"))
            _same_histogram(m, want_h)
            want = ae.Meter(**kw).update(want_h["histogram"], manual_exposure=manual)
            assert m["valid"] == want["valid"]
            d = [ae.ulps_f32(m[key], want[key]) for key in ("ev", "ev_target", "mean_log2")]
            print("%dx%d %s %s spp %d: ev %.6f target %.6f mean %.6f, ulps %s" % (W, H, setting, name, spp, m["ev"], m["ev_target"], m["mean_log2"], d))
            assert max(d) <= 2.0, (name, spp, d, m["ev"], want["ev"])
            if not want["valid"]:
                assert m["ev"] == manual
            clamped += want["valid"] and want["ev"] in (kw.get("ev_range", (-8.0, 16.0)))
    assert (clamped > 0) == (setting == "tight")     # the clamp bites in the tight setting, and only there
    r.set_auto_exposure(False)


# ---------------------------------------------------------------- 3. adaptation
def test_adaptation_follows_the_recurrence(contexts):
    W, H = 64, 32
    r = contexts(W, H)
    manual = float(r.exposure[None])
    inp = _inputs(W, H)
    frames = [inp["bright"], inp["bright"] * np.float32(40.0), inp["constant"]]
    r.set_auto_exposure(True, adapt=0.25)
    ref = ae.Meter(adapt=0.25)
    evs = []
    for k, f in enumerate(frames):
        r.reset_framebuffer()                       # de_reset does not clear the state
        m = _show(r, f, 3)
        want = ref.update(ae.meter(f, 3)["histogram"], manual)
        print("frame %d: ev %r (restatement %r), target %r (restatement %r)" % (k, m["ev"], want["ev"], m["ev_target"], float(np.float32(want["ev_target"]))))
        assert m["ev"] == want["ev"] and m["ev_target"] == float(np.float32(want["ev_target"])), k      # the sequence EQUALS the restatement's
        # the recurrence on the device's own numbers: the reported target is the f64 one rounded to f32, a quarter of which reaches the EV: 1 ulp
        if k == 0:
            assert m["ev"] == m["ev_target"]        # the first display jumps
        else:
            step = evs[-1] + 0.25 * (m["ev_target"] - evs[-1])
            assert ae.ulps_f32(m["ev"], step) <= 1.0 and m["ev"] != m["ev_target"]
        evs.append(m["ev"])
    assert len(set(evs)) == 3
    # an all-black frame keeps the EV
    r.reset_framebuffer()
    m = _show(r, np.zeros((W, H, 3), np.float32), 3)
    assert not m["valid"] and m["metered"] == 0 and m["below"] == W * H and m["ev"] == evs[-1]
    m = _show(r, frames[0], 3)                      # ... and the state it kept is the one before it
    assert m["ev"] == ref.update(ae.meter(frames[0], 3)["histogram"], manual)["ev"]
    assert ae.ulps_f32(m["ev"], evs[-1] + 0.25 * (m["ev_target"] - evs[-1])) <= 1.0
    # setting it again clears the state: a jump
    r.set_auto_exposure(True, adapt=0.25)
    m = _show(r, frames[1], 3)
    assert m["ev"] == m["ev_target"]
    # black before any state: the manual exposure, and the next metering still jumps
    r.set_auto_exposure(True, adapt=0.25)
    m = _show(r, np.zeros((W, H, 3), np.float32), 3)
    assert not m["valid"] and m["ev"] == manual
    m = _show(r, frames[2], 3)
    assert m["valid"] and m["ev"] == m["ev_target"]
    r.set_auto_exposure(False)


# ---------------------------------------------------------------- 4. the display is the unchanged transform
def _rendered(R, seed=11):
    r = R.Renderer((64, 32), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=seed)
    r.copy_textures()
    r.accumulate(4)
    return r


def _params_exposure(r):
    from digital_earth_amd import _native
    p = _native.DeParams()
    assert r._lib.de_get_params(r._h, ctypes.byref(p)) == 0
    return float(p.exposure)


def test_display_is_the_unchanged_transform_at_the_metered_ev(R):
    r = _rendered(R)
    before = _params_exposure(r)
    hdr0 = r.fetch_hdr()
    r.set_auto_exposure(True)
    on = r.fetch_image()
    m = r.metering()
    assert m["valid"] and _params_exposure(r) == before
    assert (_bits(r.fetch_hdr()) == _bits(hdr0)).all()
    _same_histogram(m, ae.meter(hdr0, 4))
    r.set_auto_exposure(False)
    assert r.auto_exposure() is None
    r.set_exposure(m["ev"])
    manual = r.fetch_image()
    assert (_bits(on) == _bits(manual)).all()
    assert m["ev"] != before and not (_bits(on) == _bits(np.zeros_like(on))).all()
    r.set_exposure(before)
    back = r.fetch_image()
    never = _rendered(R)
    assert (_bits(back) == _bits(never.fetch_image())).all()
    assert (_bits(r.fetch_hdr()) == _bits(hdr0)).all() and _params_exposure(r) == before
    never.close(); r.close()


# ---------------------------------------------------------------- 5. every display source
def _on_equals_manual(r, m):
    """The feature-on image equals the manual-exposure image at the fetched EV; leaves the feature on and the manual exposure as it was."""
    on = r.fetch_image()
    keep = float(r.exposure[None])
    r.set_auto_exposure(False)
    r.set_exposure(m["ev"])
    manual = r.fetch_image()
    r.set_exposure(keep)
    r.set_auto_exposure(True)
    assert (_bits(on) == _bits(manual)).all()


def test_meter_reads_an_adaptive_frame_with_its_tile_counts(R):
    r = R.Renderer((64, 32), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=11)
    r.set_fov(0.42)
    r.copy_textures()
    r.set_auto_exposure(True)
    for tau in TAUS:
        r.reset_framebuffer()
        r.render_adaptive(tau, 32, min_spp=4, round_spp=4)
        counts = r.tile_spp()
        if len(np.unique(counts)) >= 2:
            break
    else:
        pytest.fail("no threshold of %s spreads the tile counts" % (TAUS,))
    r.fetch_image()
    m = r.metering()
    per_pixel = np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1)
    _same_histogram(m, ae.meter(r.fetch_hdr(), per_pixel))
    assert (m["histogram"] != ae.meter(r.fetch_hdr(), int(counts.max()))["histogram"]).any()      # the frame's largest count would meter something else
    _on_equals_manual(r, m)
    r.close()


def test_meter_reads_the_denoised_mean(R):
    r = R.Renderer((64, 32), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=11)
    r.set_fov(0.42)
    r.copy_textures()
    r.set_denoise(True)
    r.set_auto_exposure(True)
    r.reset_framebuffer()
    r.accumulate(4)
    r.fetch_image()
    m = r.metering()
    _same_histogram(m, ae.meter(r.fetch_denoised_hdr(), 1))
    assert (m["histogram"] != ae.meter(r.fetch_hdr(), 4)["histogram"]).any()
    _on_equals_manual(r, m)
    r.close()


@pytest.mark.parametrize("offset_floats", [0, 3])
def test_meter_reads_a_display_source(R, offset_floats):
    """A second context's buffer as the display source; offset by one pixel (12 bytes) it is no longer 16-byte aligned: the scalar-load kernel."""
    W, H = 64, 32
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    other = R.Renderer((W, H + 8), (0, 1, 0), texture_source="constant")      # larger: the shifted window stays inside it
    r.copy_textures()
    rng = np.random.default_rng(5)
    big = (np.exp2(rng.uniform(-12.0, 4.0, (W, H + 8, 1))) * rng.uniform(0.2, 1.5, (W, H + 8, 3))).astype(np.float32)
    other.upload_hdr(big, 1)
    own = _inputs(W, H)["constant"]
    r.upload_hdr(own, 5)
    ptr, _ = other.hdr_device_pointer()
    r.set_display_source(ptr + 4 * offset_floats)
    r.set_auto_exposure(True)
    r.fetch_image()
    m = r.metering()
    flat = np.ascontiguousarray(big.transpose(1, 0, 2)).ravel()              # the device layout [H][W][3]
    seen = flat[offset_floats:offset_floats + W * H * 3].reshape(H, W, 3).transpose(1, 0, 2)
    assert (_bits(r.fetch_hdr()) == _bits(seen)).all()
    _same_histogram(m, ae.meter(seen, 5))
    assert (m["histogram"] != ae.meter(own, 5)["histogram"]).any()
    _on_equals_manual(r, m)
    r.set_display_source(None)
    r.fetch_image()
    _same_histogram(r.metering(), ae.meter(own, 5))
    r.close(); other.close()


# ---------------------------------------------------------------- 6. the pipelined window loop
def test_earth_viewer_frame_loop_pipelined_with_auto_exposure():
    from digital_earth_amd.earth_viewer import EarthViewer
    kw = dict(screen_res=(64, 32), texture_source="synthetic", texture_size=(1024, 512), seed=5)

    def script(k):
        return dict(sun_angle=0.9) if k == 2 else {}

    def viewer():
        v = EarthViewer(**kw)
        v.renderer.set_auto_exposure(True, adapt=0.5)
        return v
    a = viewer()
    sync, evs = [], []
    for k in range(6):
        sync.append(a.frame(spp=1, **script(k)).copy())
        evs.append(a.renderer.metering()["ev"])
    last = a.renderer.metering()
    b = viewer()
    got = [b.frame(spp=1, pipelined=2, **script(k)) for k in range(6)]
    assert got[0] is None and got[1] is None
    tail = b.renderer.fetch_pending(all_images=True)
    seq = [np.array(x) for x in got[2:]] + tail
    assert len(seq) == 6
    for k in range(6):
        assert (_bits(seq[k]) == _bits(sync[k])).all(), k
    assert b.finish() is None
    m = b.renderer.metering()
    assert m["ev"] == last["ev"] and m["ev_target"] == last["ev_target"] and (m["histogram"] == last["histogram"]).all()
    assert len(set(evs)) > 2                        # the exposure did move along the loop
    a.close(); b.close()


# ---------------------------------------------------------------- 7. errors
def test_every_error_answers_its_code(contexts):
    from digital_earth_amd import _native
    W, H = 64, 32
    r = contexts(W, H)
    L, h = r._lib, r._h
    r.set_auto_exposure(False)

    def settings(**kw):
        s = _native.DeAutoExposure()
        s.struct_bytes = ctypes.sizeof(s)
        s.key, s.compensation, s.ev_min, s.ev_max, s.low_fraction, s.high_fraction, s.adapt = 0.18, 0.0, -8.0, 16.0, 0.10, 0.95, 1.0
        for k, v in kw.items():
            if k == "region":
                s.region[:] = v
            else:
                setattr(s, k, v)
        return s
    m = _native.DeMetering()
    m.struct_bytes = ctypes.sizeof(m)
    assert L.de_get_metering(h, ctypes.byref(m)) == ERR_STATE                 # off
    bad = [dict(struct_bytes=44), dict(key=0.0), dict(key=-1.0), dict(key=float("nan")), dict(compensation=float("inf")), dict(ev_min=2.0, ev_max=1.0),
           dict(ev_max=float("nan")), dict(low_fraction=-0.1), dict(low_fraction=0.5, high_fraction=0.5), dict(high_fraction=1.5), dict(low_fraction=1.0, high_fraction=1.0),
           dict(low_fraction=float("nan")), dict(adapt=0.0), dict(adapt=1.5), dict(adapt=float("nan")),
           dict(region=[0, 0, W + 1, H]), dict(region=[0, 0, W, H + 1]), dict(region=[-1, 0, 8, 8]), dict(region=[8, 4, 8, 6]), dict(region=[8, 6, 12, 4]), dict(region=[0, 0, 0, 4])]
    for kw in bad:
        assert L.de_set_auto_exposure(h, ctypes.byref(settings(**kw))) == ERR_INVALID, kw
        assert r.auto_exposure() is None                                      # a refused call changes nothing
    assert L.de_set_auto_exposure(None, ctypes.byref(settings())) == ERR_INVALID
    assert L.de_get_auto_exposure(h, None) == ERR_INVALID and L.de_get_metering(h, None) == ERR_INVALID
    for kw in (dict(), dict(region=[0, 0, W, H]), dict(region=[W - 1, H - 1, W, H]), dict(low_fraction=0.0, high_fraction=1.0), dict(ev_min=3.0, ev_max=3.0)):
        assert L.de_set_auto_exposure(h, ctypes.byref(settings(**kw))) == 0, kw
    assert L.de_get_metering(h, ctypes.byref(m)) == ERR_STATE                 # on, nothing displayed yet
    r.upload_hdr(_inputs(W, H)["bright"], 2)
    r.fetch_image()
    assert L.de_get_metering(h, ctypes.byref(m)) == 0 and m.valid == 1 and m.ev == 3.0
    m.struct_bytes = 8
    assert L.de_get_metering(h, ctypes.byref(m)) == ERR_INVALID
    m.struct_bytes = ctypes.sizeof(m)
    assert L.de_set_auto_exposure(h, ctypes.byref(settings())) == 0           # set again: "before the first display" again
    assert L.de_get_metering(h, ctypes.byref(m)) == ERR_STATE
    assert L.de_set_auto_exposure(h, None) == 0
    assert L.de_get_metering(h, ctypes.byref(m)) == ERR_STATE
