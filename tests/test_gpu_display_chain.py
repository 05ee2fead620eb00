"""The display path's stage chain (csrc/de_display.h: display_chain) on the GPU: denoise -> history -> meter -> bloom -> local exposure -> display.
What the intermediate fetches and the display share is pinned here: the meter runs only when the chain goes past the bloom; every fetch hands out
exactly what the next stage reads (each stage's numpy float32 restatement applied to the previous fetch, bit for bit); which refusal wins in which
state; and the displayed image is the unchanged transform over the chain's last mean.

Every context is 48x40 at 2 samples per pixel on the synthetic stand-in maps, a uniform frame unless stated otherwise."""
import ctypes

import numpy as np
import pytest

import bloom_ref as bl
import history_ref as hr
import local_exposure_ref as lx

pytestmark = pytest.mark.gpu

W, H, SPP = 48, 40, 2
ERR_STATE = -4
BLOOM = dict(intensity=0.4, threshold=0.02)
TAUS = (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01)


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


def _renderer(R, size=(W, H)):
    r = R.Renderer(size, (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=11)
    r.set_fov(0.42)
    return r


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what=""):
    """Bit for bit, except that a NaN of the restatement asks for a NaN (of any payload)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), what
    diff = (_bits(got) != _bits(want)) & ~nan
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def _device_math(r):
    """The device's own de_log and de_pow(2, .) as the restatement's two parameters (tests/test_gpu_local_exposure.py)."""
    return dict(log=lambda x: r.debug_math(1, x), pow2=lambda e: r.debug_math(6, np.full(np.shape(e), 2.0, np.float32), e))


def _scale_of(r, ev):
    return float(r.debug_math(6, np.array([2.0], np.float32), np.array([ev], np.float32))[0])


# ---------------------------------------------------------------- 1. the meter runs only when the chain goes past the bloom
def test_intermediate_fetches_leave_the_meter_alone(R):
    def run(intermediate):
        r = _renderer(R)
        r.copy_textures()
        r.set_auto_exposure(True, adapt=0.5)      # adapt < 1: every metering moves the state, so one too many shows
        r.set_history(True)
        r.set_bloom(True, **BLOOM)
        r.set_local_exposure(True)
        r.accumulate(SPP)
        if intermediate:
            for fetch in (r.fetch_history_hdr, r.fetch_bloom_hdr):
                fetch()
                with pytest.raises(R.DigitalEarthError) as e:      # nothing has been displayed
                    r.metering()
                assert e.value.code == ERR_STATE
        r.fetch_local_exposure_hdr()
        first = r.metering()                                        # the chain went past the bloom: it metered
        r.reset_framebuffer()
        r.set_sun_angle(float(np.radians(20.0)))                    # another light: another target
        r.accumulate(SPP)
        if intermediate:
            r.fetch_history_hdr()
            r.fetch_bloom_hdr()
        r.fetch_image()
        second = r.metering()
        r.close()
        return first, second
    a1, a2 = run(True)
    b1, b2 = run(False)
    assert a1["valid"] and a2["valid"]
    assert a1["ev"] == b1["ev"] and a2["ev"] == b2["ev"]            # the adaptation state advanced once per display, not per fetch
    assert a2["ev"] != a2["ev_target"] and a2["ev"] != a1["ev"]      # and it was adapting: a metering too many would have moved it
    assert (a2["histogram"] == b2["histogram"]).all()


# ---------------------------------------------------------------- 2. every fetch hands out what the next stage reads
def _compose(r, history):
    """The three fetches of a context with history, bloom and local exposure on and auto-exposure off; history = what fetch_history_hdr must equal."""
    scale = _scale_of(r, float(r.exposure[None]))
    h = r.fetch_history_hdr()
    b = r.fetch_bloom_hdr()
    l = r.fetch_local_exposure_hdr()
    if history is not None:
        _same(h, history, "history")
    _same(b, bl.bloom(h[..., :3], 1, **BLOOM)[0], "bloom of the history's mean")
    _same(l, lx.local_exposure(b, 1, scale, **_device_math(r))[0], "local exposure of the bloom's mean")
    assert (_bits(b) != _bits(h[..., :3])).any() and (_bits(l) != _bits(b)).any()      # every stage did something
    return h, b, l


@pytest.mark.parametrize("denoise", [False, True])
def test_fetches_compose_across_a_camera_move(R, denoise):
    r = _renderer(R)
    r.copy_textures()
    r.set_denoise(denoise)
    r.set_history(True)
    r.set_bloom(True, **BLOOM)
    r.set_local_exposure(True)
    r.reset_framebuffer()
    r.accumulate(SPP)
    r.fetch_image()
    r.reset_framebuffer()                                             # what was displayed becomes the history
    look = [float(v) for v in r.look_at[None]]
    r.set_look_at(look[0] + 2.0e4, look[1], look[2])                  # a small move: most pixels find their history
    r.accumulate(SPP)
    h, b, l = _compose(r, None)
    assert (h[..., 3] > SPP).mean() > 0.5                             # the history did contribute
    if denoise:
        assert (_bits(h[..., :3]) != _bits(hr.mean_of(r.fetch_hdr(), SPP))).any()
    r.close()


def test_fetches_compose_on_an_adaptive_frame(R):
    """per_tile is true into the first stage (the history divides every tile by its own count) and false after it."""
    r = _renderer(R)
    r.copy_textures()
    for tau in TAUS:
        r.reset_framebuffer()
        r.render_adaptive(tau, 32, min_spp=4, round_spp=4)
        counts = r.tile_spp()
        if len(np.unique(counts)) >= 2:
            break
    else:
        pytest.fail("no threshold of %s spreads the tile counts" % (TAUS,))
    per_pixel = np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1)
    r.set_history(True)
    r.set_bloom(True, **BLOOM)
    r.set_local_exposure(True)
    hdr = r.fetch_hdr()
    want = hr.blend(hr.mean_of(hdr, per_pixel), per_pixel, r.fetch_guides()[..., 1], None)      # no history yet: the mean and its count
    h, b, l = _compose(r, want)
    assert (_bits(h[..., :3]) != _bits(hr.mean_of(hdr, int(counts.max())))).any()               # the frame's largest count would give something else
    r.close()


# ---------------------------------------------------------------- 3. which refusal wins
def _bare(R, maps=(0, 1, 2, 3, 4, 5, 6), luts=True):
    """A context holding only the given maps and, or not, the LUTs."""
    r = _renderer(R)
    for item in r._texture_plan:
        if item[1] in maps:
            r._copy_one(item)
    if luts:
        cie, s2s, o3, crf = r._luts
        R.check(r._lib.de_upload_luts(r._h, cie.ctypes.data, s2s.ctypes.data, o3.ctypes.data, crf.ctypes.data, crf.shape[1]))
    r._textures_copied = True                                         # no fetch of the Python layer uploads what the state leaves out
    return r


FETCHES = {"denoised": ("de_fetch_denoised_hdr", 3), "history": ("de_fetch_history_hdr", 4), "bloom": ("de_fetch_bloom_hdr", 3),
           "local exposure": ("de_fetch_local_exposure_hdr", 3), "image": ("de_fetch_image", 3)}
STAGE_ON = {"denoised": lambda r: r.set_denoise(True), "history": lambda r: r.set_history(True), "bloom": lambda r: r.set_bloom(True),
            "local exposure": lambda r: r.set_local_exposure(True), "image": lambda r: None}
OFF = {"denoised": "the denoiser is off", "history": "history reprojection is off", "bloom": "bloom is off", "local exposure": "local exposure is off"}
RENDERING_MAPS, RENDERING_LUTS = "all 7 textures must be uploaded or generated before rendering", "LUTs must be uploaded before rendering"
HISTORY_MAPS = "history reprojection takes its distances from the maps"
PARTITION = "the denoiser filters whole frames: not under a tile partition"
SAMPLE_PARTITION = "the denoiser filters whole frames: not under a sample partition"

# (fetch, state) -> (return code, what de_last_error starts with).  The library's behaviour at the commit that introduced display_chain, recorded.
TABLE = {
    ("denoised", "stage off"): (ERR_STATE, OFF["denoised"]),
    ("history", "stage off"): (ERR_STATE, OFF["history"]),
    ("bloom", "stage off"): (ERR_STATE, OFF["bloom"]),
    ("local exposure", "stage off"): (ERR_STATE, OFF["local exposure"]),
    ("denoised", "no LUTs"): (ERR_STATE, RENDERING_LUTS),                       # the guides need a render launch's arguments
    ("history", "no LUTs"): (ERR_STATE, "LUTs must be uploaded before fetch_history_hdr"),
    ("bloom", "no LUTs"): (0, None),                                             # legal: the bloom reads no frame constants
    ("local exposure", "no LUTs"): (ERR_STATE, "LUTs must be uploaded before fetch_local_exposure_hdr"),
    ("image", "no LUTs"): (ERR_STATE, "LUTs must be uploaded before fetch_image"),
    ("denoised", "a map missing"): (ERR_STATE, RENDERING_MAPS),
    ("history", "a map missing"): (ERR_STATE, HISTORY_MAPS),
    ("bloom", "a map missing"): (0, None),
    ("local exposure", "a map missing"): (0, None),
    ("image", "a map missing"): (0, None),
    ("denoised", "denoiser under a tile partition"): (ERR_STATE, PARTITION),
    ("history", "denoiser under a tile partition"): (ERR_STATE, PARTITION),
    ("bloom", "denoiser under a tile partition"): (ERR_STATE, PARTITION),
    ("local exposure", "denoiser under a tile partition"): (ERR_STATE, PARTITION),
    ("image", "denoiser under a tile partition"): (ERR_STATE, PARTITION),
    # two refusals at once: the one the entry point checks first
    ("history", "stage off, nothing uploaded"): (ERR_STATE, OFF["history"]),
    ("history", "nothing uploaded"): (ERR_STATE, HISTORY_MAPS),                  # the maps before the LUTs
    ("history", "no LUTs, denoiser under a sample partition"): (ERR_STATE, "LUTs must be uploaded before fetch_history_hdr"),
    ("local exposure", "stage off, nothing uploaded"): (ERR_STATE, OFF["local exposure"]),
    ("local exposure", "no LUTs, denoiser under a sample partition"): (ERR_STATE, "LUTs must be uploaded before fetch_local_exposure_hdr"),
    ("bloom", "no LUTs, denoiser under a sample partition"): (ERR_STATE, SAMPLE_PARTITION),
    ("denoised", "no LUTs, denoiser under a sample partition"): (ERR_STATE, SAMPLE_PARTITION),
    ("image", "no LUTs, denoiser under a sample partition"): (ERR_STATE, "LUTs must be uploaded before fetch_image"),
}


def _in_state(R, fetch, state):
    if state == "stage off":
        r = _bare(R)
        r.accumulate(1)
    elif state == "no LUTs":
        r = _bare(R, luts=False)
        STAGE_ON[fetch](r)
    elif state == "a map missing":
        r = _bare(R, maps=(0, 1, 2, 3, 4, 5))
        r.upload_hdr(np.full((W, H, 3), 0.4, np.float32), 1)
        STAGE_ON[fetch](r)
    elif state == "denoiser under a tile partition":
        r = _bare(R)
        r.set_denoise(True)
        STAGE_ON[fetch](r)
        r.set_tile_partition(0, 2)
        r.accumulate(1)
    elif state == "stage off, nothing uploaded":
        r = _bare(R, maps=(), luts=False)
    elif state == "nothing uploaded":
        r = _bare(R, maps=(), luts=False)
        STAGE_ON[fetch](r)
    elif state == "no LUTs, denoiser under a sample partition":
        r = _bare(R, luts=False)
        r.set_denoise(True)
        STAGE_ON[fetch](r)
        r.set_sample_partition(0, 2)
    else:
        raise KeyError(state)
    return r


@pytest.mark.parametrize("fetch,state", sorted(TABLE))
def test_precondition_precedence(R, fetch, state):
    code, message = TABLE[(fetch, state)]
    r = _in_state(R, fetch, state)
    name, k = FETCHES[fetch]
    out = np.empty((W, H, k), np.float32)
    rc = getattr(r._lib, name)(r._h, out.ctypes.data)
    said = r._lib.de_last_error().decode(errors="replace")
    r.close()
    assert rc == code, (rc, said)
    if message is not None:
        assert said.startswith(message), said


# ---------------------------------------------------------------- 4. the display is the unchanged transform over the chain's last mean
def test_image_is_the_display_of_the_chains_last_mean(R):
    r = _renderer(R)
    r.copy_textures()
    r.set_denoise(True)
    r.set_history(True)
    r.set_bloom(True, **BLOOM)
    r.set_local_exposure(True)
    r.reset_framebuffer()
    r.accumulate(SPP)
    image = r.fetch_image()
    last = r.fetch_local_exposure_hdr()
    plain = _renderer(R)                                              # the same parameters, every stage off
    holder = _renderer(R)
    plain.copy_textures()
    holder.upload_hdr(last, 1)
    plain.upload_hdr(np.zeros((W, H, 3), np.float32), 1)              # one sample per pixel: the source is a mean
    ptr, _ = holder.hdr_device_pointer()
    plain.set_display_source(ptr)
    assert (_bits(plain.fetch_hdr()) == _bits(last)).all()
    assert (_bits(plain.fetch_image()) == _bits(image)).all()
    r.set_denoise(False); r.set_history(False); r.set_bloom(False); r.set_local_exposure(False)
    assert (_bits(r.fetch_image()) != _bits(image)).any()            # and the stages show
    plain.set_display_source(None)
    plain.close(); holder.close(); r.close()
