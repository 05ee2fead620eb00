"""The HDR display output (include/digital_earth_hdr_output.h) on the GPU: the transform, whole frames and the packed pixels equal the numpy
float32 restatement (tests/hdr_output_ref.py, with the device's own de_pow, de_log and de_sqrt injected through Renderer.debug_math) bit for bit; the
device also meets the executed reference (tests/golden/ref_opendrt_hdr.npz) within the bounds of tests/test_hdr_output_ref.py; the stage sits where
display_kernel sat (adaptive counts, the metered exposure, bloom and local exposure ahead of it, output scaling behind it); off again, every byte is what
it was; AgX and HDR together are refused.

Sizes: 48x24 leaves partial 32x32 tiles on both axes (16 and 24 pixels); 64x32 is two whole tiles and, adaptive, 8x4 tile counts; 32x16 is the scaled
output.  Where the restatement's value is a NaN the device must hold a NaN there; everything else is compared as bits."""
import os

import numpy as np
import pytest

import hdr_output_ref as ho
from test_hdr_output_ref import compare_with_fixture

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CONFIGS = [dict(peak_nits=1000.0, gamut="rec2020", transfer="pq"), dict(peak_nits=1000.0, gamut="p3d65", transfer="hlg")]
TAUS = (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01)


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


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


def device_math(r):
    """The device's own de_pow, de_log and de_sqrt as the restatement's three parameters."""
    return dict(pow=lambda x, y: r.debug_math(6, x, y), log=lambda x: r.debug_math(1, x), sqrt=lambda x: r.debug_math(8, x))


def scale_of(r, ev):
    """exposure_scale as setup_kernel and the meter make it: de_pow(2, ev)."""
    return float(r.debug_math(6, np.array([2.0], np.float32), np.array([ev], np.float32))[0])


def vignette_of(r):
    return (r.vignette_strength, r.vignette_radius) + tuple(r.vignette_center)


def _renderer(R, size=(64, 32), seed=11):
    r = R.Renderer(size, (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=seed)
    r.set_fov(0.42)
    r.copy_textures()
    r.vignette_strength, r.vignette_radius, r.vignette_center = 0.6, 0.15, (0.4, 0.55)      # not the defaults
    r.set_exposure(3.25)
    return r


# ---------------------------------------------------------------- 1. the transform alone
def test_transform_equals_the_restatement_and_meets_the_executed_reference(R):
    z = np.load(os.path.join(GOLDEN, "ref_opendrt_hdr.npz"))
    r = R.Renderer((16, 8), (0, 1, 0), texture_source="constant")
    dm = device_math(r)
    for (peak, g, t), ref in zip(z["configs"], z["out"]):
        gamut, transfer = ho.GAMUTS[int(g)], ho.TRANSFERS[int(t)]
        got = r.debug_hdr_transform(z["rgb"], peak_nits=peak, gamut=gamut, transfer=transfer)
        _same(got, ho.transform(z["rgb"], peak, gamut, transfer, **dm), (peak, gamut, transfer))
        compare_with_fixture(got, ref, transfer)
    assert r.hdr_output is None                                               # the hook does not turn the stage on
    r.close()


# ---------------------------------------------------------------- 2. whole frames
@pytest.mark.parametrize("config", CONFIGS, ids=["pq-rec2020", "hlg-p3"])
def test_frame_with_partial_tiles(R, config):
    r = _renderer(R, (48, 24))
    r.accumulate(2)
    r.set_hdr_output(True, **config)
    got = r.fetch_image()
    want = ho.display(r.fetch_hdr(), 2, scale_of(r, 3.25), vignette_of(r), **config, **device_math(r))
    _same(got, want, config)
    assert got.shape == (48, 24, 3) and np.nanmax(got) <= 1.0 and np.nanmin(got) >= 0.0 and len(np.unique(got)) > 100
    assert r.hdr_output == dict(on=True, pixel_format="rgb10a2", mode="truncate", seed=0, animate=False, last_phase=0, **config)
    r.close()


@pytest.mark.parametrize("config", CONFIGS, ids=["pq-rec2020", "hlg-p3"])
def test_adaptive_frame_is_divided_by_its_tile_counts(R, config):
    r = _renderer(R)
    for tau in TAUS:
        r.reset_framebuffer()
        r.render_adaptive(tau, 32, min_spp=4, round_spp=4)
        counts = r.tile_spp()
        if len(np.unique(counts)) >= 2:
            break
    else:
        pytest.fail("no threshold of %s spreads the tile counts" % (TAUS,))
    r.set_hdr_output(True, **config)
    got = r.fetch_image()
    per_pixel = np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1)
    hdr, scale, dm = r.fetch_hdr(), scale_of(r, 3.25), device_math(r)
    _same(got, ho.display(hdr, per_pixel, scale, vignette_of(r), **config, **dm), config)
    assert (_bits(got) != _bits(ho.display(hdr, int(counts.max()), scale, vignette_of(r), **config, **dm))).any()      # the frame's largest count would give something else
    r.close()


def test_stage_sits_behind_the_meter_the_bloom_and_the_local_exposure(R):
    r = _renderer(R)
    r.accumulate(2)
    r.set_auto_exposure(True)
    r.set_bloom(True, intensity=0.3)
    r.set_local_exposure(True)
    r.set_hdr_output(True)
    got = r.fetch_image()
    ev = r.metering()["ev"]
    assert ev != 3.25
    dodged = r.fetch_local_exposure_hdr()                                      # the display chain up to the transform, a mean
    assert r.metering()["ev"] == ev                                           # adapt = 1: metering again changes nothing
    _same(got, ho.display(dodged, 1, scale_of(r, ev), vignette_of(r), **device_math(r)))
    assert (_bits(got) != _bits(ho.display(r.fetch_hdr(), 2, scale_of(r, 3.25), vignette_of(r), **device_math(r)))).any()
    r.close()


def test_output_scaling_resamples_the_signal(R):
    r = _renderer(R)
    r.accumulate(2)
    r.set_hdr_output(True, pixel_format="rgb16", mode="round")
    full = r.fetch_image()
    r.set_output_scale((32, 16))
    got = r.fetch_image()
    assert got.shape == (32, 16, 3)
    _same(got, r.debug_output_scale(full, (32, 16)))
    px = r.fetch_hdr_pixels()
    assert px.shape == (16, 32, 3) and px.dtype == np.uint16 and (px == ho.pack(got, "rgb16", "round")).all()
    r.set_hdr_output(True)
    px = r.fetch_hdr_pixels()
    assert px.shape == (16, 32) and px.dtype == np.uint32 and (px == ho.pack(got, "rgb10a2", "truncate")).all()
    r.close()


# ---------------------------------------------------------------- 3. the pixels
def test_pixels_in_both_formats_and_three_modes(R):
    r = _renderer(R, (48, 24))
    r.accumulate(2)
    r.set_hdr_output(True)
    image = r.fetch_image()
    for fmt in ho.FORMATS:
        for mode in ho.MODES:
            r.set_hdr_output(True, pixel_format=fmt, mode=mode, seed=123)
            px = r.fetch_hdr_pixels()
            assert (px == ho.pack(image, fmt, mode, seed=123, phase=0)).all(), (fmt, mode)
            assert (r.fetch_hdr_pixels() == px).all() and r.hdr_output["last_phase"] == 0      # animate=False: the same bytes again
    r.set_hdr_output(True, pixel_format="rgb16", mode="dither", seed=123, animate=True)
    first, second = r.fetch_hdr_pixels(), r.fetch_hdr_pixels()
    assert (first == ho.pack(image, "rgb16", "dither", seed=123, phase=0)).all() and (second == ho.pack(image, "rgb16", "dither", seed=123, phase=1)).all()
    assert (first != second).any() and r.hdr_output["last_phase"] == 1
    # 8 bits of the same signal: legal, coarse
    assert (r.fetch_pixels() == r.debug_pixels(image)).all()
    # black and the clip in display-linear light: half the frame far above the shoulder (exactly 1.0), half of it unlit (a signal of about 1e-9)
    sums = np.zeros((48, 24, 3), np.float32)
    sums[:24] = 1e9
    r.upload_hdr(sums, 1)
    for fmt in ho.FORMATS:
        for mode in ho.MODES:
            r.set_hdr_output(True, transfer="linear", pixel_format=fmt, mode=mode, seed=9, animate=True)
            signal = r.fetch_image()
            assert (signal[:24] == 1.0).all() and (signal[24:] < 1e-6).all()
            px = r.fetch_hdr_pixels()
            assert (px == ho.pack(signal, fmt, mode, seed=9, phase=0)).all(), (fmt, mode)
            codes = px if fmt == "rgb16" else np.stack([px & 1023, (px >> 10) & 1023, (px >> 20) & 1023], axis=-1)
            assert (codes[:, :24] == ho.MAXCODE[fmt]).all() and (codes[:, 24:] == 0).all(), (fmt, mode)      # the picture's columns are u
            if fmt == "rgb10a2":
                assert ((px >> 30) == 3).all()
    r.close()


# ---------------------------------------------------------------- 4. no side effects, and the refusal
def test_off_again_every_byte_is_what_it_was(R):
    r = _renderer(R)
    r.accumulate(2)
    hdr0, image0, pixels0 = r.fetch_hdr(), r.fetch_image(), r.fetch_pixels()
    assert r.hdr_output is None
    with pytest.raises(R.DigitalEarthError) as e:
        r.fetch_hdr_pixels()
    assert e.value.code == -4
    r.set_hdr_output(True)
    on = r.fetch_image()
    r.fetch_hdr_pixels()
    assert (_bits(on) != _bits(image0)).any() and (_bits(r.fetch_hdr()) == _bits(hdr0)).all()
    r.set_hdr_output(False)
    assert r.hdr_output is None
    assert (_bits(r.fetch_image()) == _bits(image0)).all() and (r.fetch_pixels() == pixels0).all() and (_bits(r.fetch_hdr()) == _bits(hdr0)).all()
    fresh = _renderer(R)                                                      # a context that never heard of the stage
    fresh.accumulate(2)
    assert (_bits(fresh.fetch_image()) == _bits(image0)).all() and (fresh.fetch_pixels() == pixels0).all()
    for kw in (dict(peak_nits=99.0), dict(peak_nits=float("nan")), dict(peak_nits=20000.0)):
        with pytest.raises(R.DigitalEarthError) as e:
            r.set_hdr_output(True, **kw)
        assert e.value.code == -1 and r.hdr_output is None                   # a refused call changes nothing
    fresh.close(); r.close()


def test_agx_and_hdr_together_are_refused(R):
    r = _renderer(R)
    r.accumulate(1)
    r.set_display_transform("agx")
    sdr = r.fetch_image()
    r.set_hdr_output(True)
    for call in (r.fetch_image, r.fetch_hdr_pixels, r.fetch_pixels):
        with pytest.raises(R.DigitalEarthError) as e:
            call()
        assert e.value.code == -4
    r.set_hdr_output(False)
    assert (_bits(r.fetch_image()) == _bits(sdr)).all()
    r.set_display_transform("opendrt")
    r.set_hdr_output(True)
    assert np.isfinite(r.fetch_image()).all()
    r.close()


def test_earth_viewer_frames_and_saves_hdr(R, tmp_path):
    import struct
    import zlib
    from digital_earth_amd.earth_viewer import EarthViewer
    v = EarthViewer(screen_res=(64, 32), hdr_output=dict(transfer="hlg", gamut="p3d65", pixel_format="rgb16"), texture_source="synthetic", texture_size=(1024, 512), seed=5)
    assert v.renderer.hdr_output["transfer"] == "hlg"
    px = v.frame(spp=1, hdr_pixels=True)
    assert px.shape == (32, 64, 3) and px.dtype == np.uint16
    path = str(tmp_path / "shot.png")
    v.save(path)
    data = open(path, "rb").read()
    assert struct.unpack(">IIBB", data[16:26]) == (64, 32, 16, 2)
    assert data[33:41] == struct.pack(">I", 4) + b"cICP" and tuple(data[41:45]) == (12, 18, 0, 1)
    n = struct.unpack(">I", data[49:53])[0]
    raw = np.frombuffer(zlib.decompress(data[57:57 + n]), np.uint8).reshape(32, 1 + 64 * 6)
    assert (raw[:, 1:].copy().view(">u2").reshape(32, 64, 3) == px).all()
    # saving displays nothing and touches no setting: 10-bit codes are widened, a float signal is rounded on the host, each labelled as it was taken
    from digital_earth_amd import png16
    r = v.renderer
    r.set_hdr_output(True, transfer="pq", gamut="rec2020", pixel_format="rgb10a2", mode="dither", seed=4, animate=True)
    ten = v.frame(spp=1, hdr_pixels=True)
    signal = v.frame(spp=1)
    before = r.hdr_output
    assert before["last_phase"] == 0
    r.set_hdr_output(True, transfer="hlg", gamut="p3d65", animate=True)                       # a later change of the settings does not relabel the held picture
    for held, name in ((signal, "b.png"), (None, "c.png")):
        if held is None:
            v._pixels, v._image = ten, None
        v.save(str(tmp_path / name))
        data = open(str(tmp_path / name), "rb").read()
        assert tuple(data[41:45]) == (9, 16, 0, 1)
        n = struct.unpack(">I", data[49:53])[0]
        raw = np.frombuffer(zlib.decompress(data[57:57 + n]), np.uint8).reshape(32, 1 + 64 * 6)
        assert (raw[:, 1:].copy().view(">u2").reshape(32, 64, 3) == png16.to_rgb16(ten if held is None else signal)).all()
    assert r.hdr_output["last_phase"] == 0 and r.hdr_output["transfer"] == "hlg"             # no conversion ran, nothing was reset
    # a pipelined loop hands out an earlier iteration's picture: its label is that iteration's setting, through frame() and through finish()
    assert v.frame(spp=1, pipelined=1) is None                                                 # taken under HLG / P3
    r.set_hdr_output(True, transfer="pq", gamut="rec709")
    first = v.frame(spp=1, pipelined=1)                                                        # taken under PQ / Rec.709, returns the HLG picture
    assert first is not None and v._held_hdr["transfer"] == "hlg" and v._held_hdr["gamut"] == "p3d65"
    v.save(str(tmp_path / "d.png"))
    assert tuple(open(str(tmp_path / "d.png"), "rb").read()[41:45]) == (12, 18, 0, 1)
    r.set_hdr_output(True, transfer="linear", gamut="rec2020")
    last = v.finish()
    assert last is not None and v._held_hdr["transfer"] == "pq" and v._held_hdr["gamut"] == "rec709" and v._hdr_in_flight == {False: [], True: []}
    v.save(str(tmp_path / "e.png"))
    assert tuple(open(str(tmp_path / "e.png"), "rb").read()[41:45]) == (1, 16, 0, 1)
    v.close()
