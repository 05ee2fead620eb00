"""The shared deflate coder (csrc/png_deflate.h: png_code_chunk, instantiated in png_deflate_kernel and exr_deflate_kernel) on the
GPU at the edges the cases of tests/png_cases.py and tests/exr_cases.py never reach (tests/deflate_cases.py; tests/test_deflate_cases.py proves on
the CPU that each input reaches its branch): the 15-bit length limit, chunks of the full 65 535 bytes, every length code, chunk lengths around the
512-thread split.  Each file equals the numpy restatement byte for byte AND, checked apart from that, decodes to its input through zlib — so a
failure says which side is wrong.  Two contexts run the shipped default chunk, filled, through the ring's fetch path."""
import numpy as np
import pytest

import deflate_cases as dc
import exr_ref as xr
import png_ref as pr
from digital_earth_amd import exr

pytestmark = pytest.mark.gpu

F = np.float32
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


def _same(got, want, what=""):
    got, want = bytes(got), bytes(want)
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("%s: GPU against the restatement: %d bytes against %d, first difference at %d" % (what, len(got), len(want), first))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _sums(W, H, seed):
    """Accumulated sums as tests/test_gpu_png.py uploads them: a few decades of exposure, a black corner."""
    rng = np.random.default_rng(seed)
    s = (np.exp2(rng.uniform(-9.0, 3.0, (W, H, 1))) * rng.uniform(0.3, 1.6, (W, H, 3))).astype(F)
    s[: W // 4, : H // 4] = 0.0
    return s


# ---------------------------------------------------------------- 1. the kernels, byte for byte
@pytest.mark.parametrize("name", sorted(dc.PNG_CASES))
def test_png_equals_the_restatement_and_inflates_to_the_input(ctx, name):
    px, flt, chunk = dc.PNG_CASES[name]
    before = ctx.png()
    got = ctx.debug_png(px, filter=flt, chunk_bytes=chunk)
    failures = []
    try:
        _same(got, dc.png_encoded(name)[0], name)
    except AssertionError as e:
        failures.append(str(e))
    try:                                                           # on its own: zlib judges the GPU's file whatever the restatement says
        back, info = pr.decode(got)
        assert back.dtype == px.dtype and np.array_equal(back, px), "%s: the GPU's file inflates to other pixels" % name
    except Exception as e:
        failures.append("%s: GPU against zlib: %s: %s" % (name, type(e).__name__, e))
    assert not failures, "; ".join(failures)
    assert len(got) <= pr.capacity(px.shape[1], px.shape[0], px.shape[2], 8 * px.dtype.itemsize, chunk)
    assert ctx.png() == before                                     # the debug entry point leaves the context's settings alone


@pytest.mark.parametrize("name", sorted(dc.EXR_CASES))
def test_exr_equals_the_restatement_and_reads_back(ctx, name):
    image, pixel_type, compression, chunk, scale = dc.EXR_CASES[name]
    before = ctx.exr()
    got = ctx.debug_exr(image, pixel_type=pixel_type, compression=compression, chunk_bytes=chunk, scale=scale)
    want, blocks = dc.exr_encoded(name)
    failures = []
    try:
        _same(got, want, name)
    except AssertionError as e:
        failures.append(str(e))
    try:
        back, info = exr.read(got)
        assert np.array_equal(_bits(back), _bits(xr.convert(image, scale, pixel_type))), "%s: the GPU's file reads back as other samples" % name
        assert [("raw" if b["raw"] else "zip") for b in info["blocks"]] == list(blocks)
    except Exception as e:
        failures.append("%s: GPU against zlib: %s: %s" % (name, type(e).__name__, e))
    assert not failures, "; ".join(failures)
    assert len(got) <= xr.capacity(image.shape[1], image.shape[0], pixel_type, compression)
    assert ctx.exr() == before


# ---------------------------------------------------------------- 2. the shipped default chunk, filled, through the ring's fetch path
def test_png_frame_fills_a_default_chunk(R):
    PW, PH = 128, 96                                               # 96 (1 + 384) = 36 960 filtered bytes: a full chunk of 32 768 and one of 4 192
    r = R.Renderer((PW, PH), (0, 1, 0), texture_source="constant")
    try:
        r.copy_textures()
        r.upload_hdr(_sums(PW, PH, 41), 3)
        r.set_pixels(3, "round")
        r.set_png()
        assert r.png()["chunk_bytes"] == pr.DEFAULT_CHUNK == 32768 and PH * (1 + 3 * PW) == 36960
        px = r.fetch_pixels().copy()
        got = r.fetch_png()
        info = []
        want = pr.encode(px, info=info)
        assert len(info) == 2
        _same(got, want, "fetch_png at the default chunk")
        assert np.array_equal(pr.decode(got)[0], px)
        assert r.fetch_png(lag=1) is None                          # and the ring's cell: the same bytes
        _same(r.fetch_pending_png(), want, "the lagged fetch at the default chunk")
    finally:
        r.close()


def test_exr_frame_fills_a_default_chunk(R):
    EW, EH = 352, 16                                               # one HALF block of 352 * 16 * 6 = 33 792 bytes: pieces of 32 768 and 1 024
    r = R.Renderer((EW, EH), (0, 1, 0), texture_source="constant")
    try:
        r.copy_textures()
        r.upload_hdr(_sums(EW, EH, 42), 3)
        r.set_exr()
        assert r.exr()["chunk_bytes"] == xr.DEFAULT_CHUNK == 32768 and r.exr()["pixel_type"] == "half" and r.exr()["compression"] == "zip"
        want_image = np.ascontiguousarray((r.fetch_hdr() / F(r.current_spp))[:, ::-1].transpose(1, 0, 2))      # rows top-down, as tests/test_gpu_exr.py
        assert want_image.dtype == F and want_image.size * 2 == 33792
        got = r.fetch_exr()
        want = xr.encode(want_image, "half", "zip")
        _same(got, want, "fetch_exr at the default chunk")
        back, info = exr.read(got)
        assert np.array_equal(_bits(back), _bits(xr.convert(want_image, 1.0, "half"))) and len(info["blocks"]) == 1
        assert r.fetch_exr(lag=1) is None
        _same(r.fetch_pending_exr(), want, "the lagged fetch at the default chunk")
    finally:
        r.close()
