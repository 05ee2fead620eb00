"""The HDR display output without a GPU: the numpy restatement (tests/hdr_output_ref.py, numpy's own float32 power / logarithm) against the
reference's text executed in five configurations (tests/golden/ref_opendrt_hdr.npz, written by tools/ref_fixtures/make_hdr.py), closed-form anchors of
ST 2084, the pack's exact ends and bit layout, and the 16-bit PNG writer's round trip.

Bounds.  The two linear configurations are held to the bound the suite holds the `opendrt` leaf to against ref_leaves.npz (tests/test_ref_fixtures.py:
largest absolute difference <= 1e-6 of the largest |value|); the live one, (100, Rec709, lin), shares its inputs and outputs with that leaf.  For PQ and HLG
the largest absolute difference between the restatement and the executed reference was MEASURED here, on the CPU, where both sides call the same libm:
    PQ   6.02e-6  ((1000, Rec2020, pq); (600, Rec709, pq) agrees in every bit)
    HLG  2.68e-7  ((1000, P3D65, hlg))
and four times those figures are asserted.  The differences come from the constants (host double rounded once here, f32 step by step in the reference's
locals): one ulp of the clamped display-linear value enters pow(., 2523/32 = 78.84), which multiplies it by about 79."""
import os
import struct
import zlib

import numpy as np
import pytest

import hdr_output_ref as ho

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEASURED = {"pq": 6.02e-6, "hlg": 2.68e-7}      # largest |restatement - executed reference| on the CPU (this file's docstring)
BOUND = {t: 4.0 * v for t, v in MEASURED.items()}
LEAF_BOUND = 1e-6                                # tests/test_ref_fixtures.py LEAVES["opendrt"]: abs, relative to the largest |value|


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "ref_opendrt_hdr.npz"))
    return z["rgb"], z["out"], [(float(p), ho.GAMUTS[int(g)], ho.TRANSFERS[int(t)]) for p, g, t in z["configs"]]


def compare_with_fixture(got, want, transfer):
    """The check of one configuration: rows where either side is not finite are compared for the class of every value and may be 2 % of the rows at
    most; the others within the transfer's bound.  Returns the largest absolute difference."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    out = ~(np.isfinite(got).all(axis=1) & np.isfinite(want).all(axis=1))
    assert out.mean() <= 0.02, out.sum()
    assert (np.isnan(got[out]) == np.isnan(want[out])).all() and (np.isposinf(got[out]) == np.isposinf(want[out])).all() and (np.isneginf(got[out]) == np.isneginf(want[out])).all()
    worst = float(np.abs(got[~out].astype(np.float64) - want[~out]).max())
    bound = LEAF_BOUND * float(np.abs(want[~out]).max()) if transfer == "linear" else BOUND[transfer]
    print("transfer %s: largest absolute difference %.3g (bound %.3g), %d rows not finite" % (transfer, worst, bound, int(out.sum())))
    assert worst <= bound, (transfer, worst, bound)
    return worst


def test_fixture_holds_the_five_configurations(fixture):
    rgb, out, configs = fixture
    assert rgb.shape == (260, 3) and out.shape == (5, 260, 3) and rgb.dtype == np.float32 and out.dtype == np.float32
    assert configs == [(100.0, "rec709", "linear"), (1000.0, "rec2020", "pq"), (1000.0, "p3d65", "hlg"), (600.0, "rec709", "pq"), (4000.0, "rec2020", "linear")]
    assert (rgb[256:] == np.array([(0, 0, 0), (0.18, 0.18, 0.18), (1e4, 1e4, 1e4), (1e3, 0, 0)], np.float32)).all()
    leaves = np.load(os.path.join(GOLDEN, "ref_leaves.npz"))
    assert (rgb[:256] == leaves["opendrt_in"]).all()                                    # the leaf's own colours ...
    assert (out[0, :256].view(np.uint32) == leaves["opendrt_out"].view(np.uint32)).all()      # ... and patching the constants back gives the leaf's own bits
    assert os.path.getsize(os.path.join(GOLDEN, "ref_opendrt_hdr.npz")) < 64 * 1024


@pytest.mark.parametrize("index", range(5))
def test_restatement_matches_the_executed_reference(fixture, index):
    rgb, out, configs = fixture
    peak, gamut, transfer = configs[index]
    got = ho.transform(rgb, peak, gamut, transfer)
    compare_with_fixture(got, out[index], transfer)


def test_live_configuration_meets_the_leaf_bound_against_ref_leaves(fixture):
    rgb, _, _ = fixture
    leaves = np.load(os.path.join(GOLDEN, "ref_leaves.npz"))
    got = ho.transform(leaves["opendrt_in"], 100.0, "rec709", "linear")
    ref = leaves["opendrt_out"]
    assert (np.isnan(ref) == np.isnan(got)).all()
    assert float(np.nanmax(np.abs(got.astype(np.float64) - ref)) / np.nanmax(np.abs(ref))) <= LEAF_BOUND


PQ_MEASURED_REL = 3.05e-6      # largest relative distance of the f32 evaluation from the float64 closed form over 0 / 100 / 600 / 1000 / 4000 / 10000 nits (at 1000: 38 ulp)


def _pq_f32_tolerance(closed):
    """How far an f32 evaluation of ST 2084 may lie from the float64 closed form.  The f32 ROUNDING of the closed form cannot be reached: the argument
    of the outer power, (c1 + c2 a) / (1 + c3 a), is itself rounded to f32 (half an ulp = 3e-8 relative at best, up to about 2.6 ulp over its two
    products, two sums and the quotient), and the exponent 2523 / 32 = 78.84 multiplies that: 2.4e-6 relative already for a perfectly rounded
    argument.  Measured, numpy float32 against float64: 1.1e-6 / 4.9e-7 / 3.05e-6 / 1.06e-6 at 100 / 600 / 1000 / 4000 nits, 6e-8 at black, 0 at
    10000.  Four times the largest figure is asserted, as for the fixture."""
    return closed * 4.0 * PQ_MEASURED_REL


def test_pq_anchors_at_f32_rounding_of_the_closed_forms():
    for nits, four_digits in ((100.0, 0.5081), (1000.0, 0.7518), (10000.0, 1.0)):
        closed = ho.pq_nits(nits)
        assert abs(closed - four_digits) < 5e-5
        got = ho.pq_inverse_eotf(np.array([nits / 10000.0], np.float32))[0]
        assert abs(float(got) - closed) <= _pq_f32_tolerance(closed), (nits, got, closed)
    assert ho.pq_inverse_eotf(np.array([1.0], np.float32))[0] == np.float32(1.0)
    assert abs(float(ho.pq_inverse_eotf(np.array([0.0], np.float32))[0]) - ho.pq_nits(0.0)) <= _pq_f32_tolerance(ho.pq_nits(0.0))      # black is code 0 of 10 bits, 0.05 of 16


@pytest.mark.parametrize("peak", [100.0, 600.0, 1000.0, 4000.0, 10000.0])
def test_clamp_max_encodes_to_pq_of_the_peak(peak):
    k = ho.constants(peak, "rec2020", "pq")
    assert k["clamp_max"] == np.float32(peak / 10000.0) and k["ds"] == np.float32(0.01)
    white = ho.transform(np.array([[1e6, 1e6, 1e6]], np.float32), peak, "rec2020", "pq")[0]
    assert (white == ho.pq_inverse_eotf(np.array([k["clamp_max"]], np.float32))[0]).all()      # a scene far above the shoulder sits on the clamp
    assert abs(float(white[0]) - ho.pq_nits(peak)) <= _pq_f32_tolerance(ho.pq_nits(peak))
    assert ho.constants(peak, "rec2020", "hlg")["clamp_max"] == np.float32(peak / 1000.0)
    assert ho.constants(peak, "rec2020", "linear")["clamp_max"] == np.float32(1.0)


def test_restated_constants_at_100_nits_are_the_live_configurations():
    """The RESTATEMENT's constants against opendrt_consts' formulas written out for Lp = 100, gb = 0.12, c = 1, fl = 0.005, dch = 0.35, EOTF = lin.  The
    library's own two host functions are put side by side in tests/test_hdr_output_abi.py::test_host_constants_at_100_nits_equal_todays_opendrt_consts."""
    import math
    gy = 11.696 / 100.0 * (1.0 + 0.12 * math.log10(1.0) / math.log10(2.0))
    s0 = (gy + math.sqrt(gy * (0.02 + gy))) / 2.0
    m0 = (1.0 + math.sqrt(1.0 * (0.02 + 1.0))) / 2.0
    px = 128.0 * math.log10(100.0) / math.log10(100.0) - 64.0
    s = (px * 0.18 * (m0 - s0)) / (px * s0 - 0.18 * m0)
    m = m0 * (s + px) / px
    k = ho.constants(100.0, "rec709", "linear")
    want = dict(m=m, s=s, fl=0.005, ds=1.0, clamp_max=1.0, dch_s=0.35 / s)
    for name, v in want.items():
        assert k[name] == np.float32(v), name
    assert (k["xyz_to_display"] == np.array(ho.XYZ_TO["rec709"], np.float32)).all()
    assert k["h_e"] == np.float32((1.0 - 1.2) / 1.2) and k["h_b"] == np.float32(1.0 - 4.0 * 0.17883277)


def test_display_gamut_products_follow_the_reference_and_are_not_colorimetric_beyond_rec709(fixture):
    """A KNOWN property of the reference's text, pinned so that it is a fact and not an accident.  lib/OpenDRT.py:86-88 multiplies `v @ m`, a row vector
    times the matrices as written — each product is by the TRANSPOSE of the colorimetric matrix.  For Rec.709 the two transposes cancel
    ((M1 M2)^T = I); for P3-D65 and Rec.2020 they do not, so neutrals leave the grey axis (towards green) there.  The stage follows the reference; only
    the Rec.709 gamut is colorimetrically meaningful as the reference stands."""
    rgb, out, configs = fixture
    one = [np.ones(1, np.float32)] * 3
    through = {g: np.array([float(c[0]) for c in ho._vdot(ho.XYZ_TO[g], ho._vdot(ho.REC709_TO_XYZ, one))]) for g in ho.GAMUTS}
    assert np.abs(through["rec709"] - 1.0).max() < 1e-6
    assert np.allclose(through["p3d65"], (0.661, 1.409, 0.920), atol=1e-3) and np.allclose(through["rec2020"], (0.333, 1.646, 0.989), atol=1e-3)
    A = np.array(ho.REC709_TO_XYZ).reshape(3, 3)
    for g in ho.GAMUTS:                                                               # the colorimetric orientation would keep white white in every gamut
        assert np.abs(np.array(ho.XYZ_TO[g]).reshape(3, 3) @ A @ np.ones(3) - 1.0).max() < 1e-6
    assert (rgb[257] == np.float32(0.18)).all()
    grey = {c: out[k, 257] for k, c in enumerate(configs)}                            # the executed reference's 0.18 grey
    assert np.ptp(grey[(100.0, "rec709", "linear")]) < 1e-6 and np.ptp(grey[(600.0, "rec709", "pq")]) == 0
    assert np.allclose(grey[(1000.0, "rec2020", "pq")], (0.2561, 0.3830, 0.3392), atol=1e-4)
    assert np.allclose(grey[(1000.0, "p3d65", "hlg")], (0.2508, 0.3647, 0.2951), atol=1e-4)
    assert np.allclose(grey[(4000.0, "rec2020", "linear")], (0.00161, 0.00790, 0.00475), atol=1e-5)
    assert np.allclose(ho.transform(np.full((1, 3), 0.18, np.float32), 1000.0, "rec2020", "linear")[0], (0.0056, 0.0267, 0.0161), atol=1e-4)


def test_pack_ends_are_exact_and_the_bits_lie_where_the_header_says():
    W, H = 16, 8
    rng = np.random.default_rng(3)
    image = rng.uniform(-0.2, 1.2, (W, H, 3)).astype(np.float32)
    image[0, 0] = (0.0, -0.0, np.nan); image[1, 0] = (1.0, np.inf, 2.0); image[2, 0] = (-np.inf, 1e-30, np.nextafter(np.float32(1), np.float32(0)))
    for fmt in ho.FORMATS:
        mc = ho.MAXCODE[fmt]
        for mode in ho.MODES:
            for seed, phase in ((0, 0), (77, 5)):
                q = ho.quantise(image, mc, mode, seed, phase, ho.pixels_ref.indices(W, H))
                assert (q[image >= 1] == mc).all() and (q[~(image > 0)] == 0).all() and q.min() >= 0 and q.max() <= mc
        px = ho.pack(image, fmt, "round")
        q = ho.quantise(image, mc, "round").transpose(1, 0, 2)[::-1]
        if fmt == "rgb16":
            assert px.dtype == np.uint16 and px.shape == (H, W, 3) and (px == q).all()
        else:
            assert px.dtype == np.uint32 and px.shape == (H, W)
            assert ((px & 1023) == q[..., 0]).all() and (((px >> 10) & 1023) == q[..., 1]).all() and (((px >> 20) & 1023) == q[..., 2]).all() and ((px >> 30) == 3).all()
    assert ho.pack(np.full((16, 8, 3), 0.5, np.float32), "rgb10a2", "truncate")[0, 0] == (511 | (511 << 10) | (511 << 20) | (3 << 30))
    assert (ho.pack(np.full((16, 8, 3), 0.5, np.float32), "rgb16", "round") == 32768).all()
    row = np.zeros((16, 8, 3), np.float32); row[3, 7] = (1.0, 0.0, 0.0)                   # the top row of the picture is v = H - 1, x = u
    assert ho.pack(row, "rgb10a2")[0, 3] == (1023 | (3 << 30))


def test_png_writer_round_trip(tmp_path):
    from digital_earth_amd import png16
    rng = np.random.default_rng(4)
    px = rng.integers(0, 65536, (5, 7, 3)).astype(np.uint16)
    px[0, 0] = (0, 65535, 258)
    for gamut, transfer, want in (("rec2020", "pq", (9, 16, 0, 1)), ("p3d65", "hlg", (12, 18, 0, 1)), ("rec709", "linear", (1, 8, 0, 1))):
        assert png16.cicp_of(gamut, transfer) == want == (ho.CICP[0][gamut], ho.CICP[1][transfer], 0, 1)
        path = str(tmp_path / "t.png")
        png16.write_png16(path, px, want)
        data = open(path, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        chunks, at = [], 8
        while at < len(data):
            n, kind = struct.unpack(">I4s", data[at:at + 8])
            body = data[at + 8:at + 8 + n]
            assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff
            chunks.append((kind, body))
            at += 12 + n
        assert [k for k, _ in chunks] == [b"IHDR", b"cICP", b"IDAT", b"IEND"]
        assert struct.unpack(">IIBBBBB", chunks[0][1]) == (7, 5, 16, 2, 0, 0, 0)      # width, height, bit depth 16, colour type 2 (RGB), deflate, filter method 0, no interlace
        assert tuple(chunks[1][1]) == want
        raw = np.frombuffer(zlib.decompress(chunks[2][1]), np.uint8).reshape(5, 1 + 7 * 6)
        assert (raw[:, 0] == 0).all()                                                   # filter type 0 on every row
        assert (raw[:, 1:].copy().view(">u2").reshape(5, 7, 3) == px).all()
    with pytest.raises(ValueError):
        png16.encode_png16(px.astype(np.uint8), (9, 16, 0, 1))


def test_held_pictures_become_16_bit_rows_on_the_host():
    """png16.to_rgb16: what EarthViewer.save writes from the picture it holds, without a new display."""
    from digital_earth_amd import png16
    rng = np.random.default_rng(6)
    signal = rng.uniform(-0.1, 1.1, (16, 8, 3)).astype(np.float32)
    signal[0, 0] = (np.nan, 1.0, 0.0)
    assert (png16.to_rgb16(signal) == ho.pack(signal, "rgb16", "round")).all()       # a float signal: the pack's ROUND formula, transposed and flipped
    wide = ho.pack(signal, "rgb16", "dither", seed=3)
    assert png16.to_rgb16(wide) is wide
    ten = png16.to_rgb16(ho.pack(signal, "rgb10a2", "truncate"))
    codes = ho.quantise(signal, 1023, "truncate").transpose(1, 0, 2)[::-1]
    assert ten.dtype == np.uint16 and (ten == ((codes << 6) | (codes >> 4))).all() and ten.max() == 65535 and ten.min() == 0
    assert (png16.to_rgb16(np.full((2, 2, 4), 255, np.uint8)) == 65535).all()
    with pytest.raises(ValueError):
        png16.to_rgb16(np.zeros((2, 2), np.float64))
