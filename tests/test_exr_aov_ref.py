"""The restatement of the EXR AOV channels (tests/exr_aov_ref.py; include/digital_earth_exr_aovs.h) held to what is independent of
it: a multi-channel file written out by hand from the layout, the independent reader (digital_earth_amd/exr.py) and zlib.decompress on its files,
the conversions of tests/exr_ref.py on its channels bit for bit, and a float64 statement of the variance of the mean."""
import struct
import zlib

import numpy as np
import pytest

import exr_aov_ref as xa
import exr_ref as xr
from digital_earth_amd import exr

F = np.float32


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def _inputs(W, H, seed):
    """Random float32 with what goes wrong in a conversion: NaN, +-inf, negatives, beyond 65504, half-subnormals in the guides, S2 < S1 mean,
    counts of 1, 2 and mixed."""
    rng = np.random.default_rng(seed)
    image = (rng.standard_normal((H, W, 3)) * 40 + 60).astype(F)
    guides = rng.standard_normal((H, W, 9)).astype(F)
    guides[..., 1] = np.abs(guides[..., 1]) * F(3e5)              # metres: beyond 65504
    counts = rng.choice(np.array([1, 2, 3, 7, 64], F), size=(H, W)).astype(F)
    s2 = (image * image / counts[..., None] * rng.uniform(0.9, 3.0, (H, W, 3))).astype(F)      # below 1: S2 < S1 mean
    specials = np.array([np.nan, np.inf, -np.inf, -1.5, 65504.0, 65520.0, 1e9, -1e9, 3e-6, -5.9e-8, 6.1e-5, 2.98e-8, 0.0, -0.0], F)
    for a in (image, guides, s2):
        flat = a.reshape(-1)
        at = rng.choice(flat.size, size=min(flat.size, max(1, flat.size // 5)), replace=False)
        flat[at] = rng.choice(specials, size=at.size)
    return image, guides, s2, counts


def test_channel_order_is_the_byte_wise_sort():
    for mask in range(128):
        names = [n for n, _ in xa.channel_list(mask)]
        assert names == [b.decode() for b in sorted(n.encode() for n in names)] and {"B", "G", "R"} <= set(names)
        assert len(names) == 3 + sum(k for bit, k in ((1, 1), (2, 3), (4, 3), (8, 1), (16, 1), (32, 3), (64, 1)) if mask & bit)
        types = dict(xa.channel_list(mask, "half"))
        assert all(types[n] == ("float" if n in ("Z", "samples") or n.startswith("variance.") else "half") for n in names)
        assert set(dict(xa.channel_list(mask, "float")).values()) == {"float"}
    assert xa.front(5, 3, "half", "zips", 0) == xr.front(5, 3, "half", "zips") and xa.capacity(5, 3, "float", "zip", 0) == xr.capacity(5, 3, "float", "zip")


def test_a_2x2_file_written_out_by_hand():
    """depth | coverage at HALF, uncompressed: the channels B, G, R, Z, coverage; Z is FLOAT among HALF planes."""
    image = np.array([[(1, 2, 3), (0.5, 0, -1)], [(4, 0.25, 70000.0), (2, 1, 0)]], F)
    guides = np.zeros((2, 2, 9), F)
    guides[..., 1] = [[100000.0, 0.0], [1.5, np.nan]]            # Z
    guides[..., 0] = [[1.0, 0.0], [0.5, 0.25]]                   # coverage
    h, f = (lambda *v: struct.pack("<%de" % len(v), *v)), (lambda *v: struct.pack("<%df" % len(v), *v))

    def ch(name, ptype):
        return name + b"\0" + struct.pack("<iB3xii", ptype, 0, 1, 1)
    chlist = ch(b"B", 1) + ch(b"G", 1) + ch(b"R", 1) + ch(b"Z", 2) + ch(b"coverage", 1) + b"\0"
    box = struct.pack("<4i", 0, 0, 1, 1)
    head = (b"\x76\x2f\x31\x01\x02\x00\x00\x00" + b"channels\0chlist\0" + struct.pack("<i", len(chlist)) + chlist
            + b"compression\0compression\0" + struct.pack("<i", 1) + b"\0"
            + b"dataWindow\0box2i\0" + struct.pack("<i", 16) + box + b"displayWindow\0box2i\0" + struct.pack("<i", 16) + box
            + b"lineOrder\0lineOrder\0" + struct.pack("<i", 1) + b"\0" + b"pixelAspectRatio\0float\0" + struct.pack("<if", 4, 1.0)
            + b"screenWindowCenter\0v2f\0" + struct.pack("<iff", 8, 0.0, 0.0) + b"screenWindowWidth\0float\0" + struct.pack("<if", 4, 1.0) + b"\0")
    line0 = h(3, -1) + h(2, 0) + h(1, 0.5) + f(100000.0, 0.0) + h(1.0, 0.0)
    line1 = h(65504.0, 0) + h(0.25, 1) + h(4, 2) + f(1.5, 0.0) + h(0.5, 0.25)      # 70000 clamps; the NaN is +0
    assert len(line0) == len(line1) == 2 * (2 + 2 + 2 + 4 + 2) and len(chlist) == 3 * 18 + 18 + 25 + 1
    at0 = len(head) + 16
    want = head + struct.pack("<QQ", at0, at0 + 8 + len(line0)) + struct.pack("<ii", 0, len(line0)) + line0 + struct.pack("<ii", 1, len(line1)) + line1
    got = xa.encode(image, guides, mask=xa.BITS["depth"] | xa.BITS["coverage"], pixel_type="half", compression="none")
    assert got == want
    back, info = exr.read(want)
    assert info["channel_names"] == ["B", "G", "R", "Z", "coverage"] and info["channel_types"]["Z"] == "float" and info["channel_types"]["coverage"] == "half"
    assert np.array_equal(info["channels"]["Z"], np.array([[100000.0, 0.0], [1.5, 0.0]], F)) and info["channels"]["Z"].dtype == F
    assert np.array_equal(back, np.array([[(1, 2, 3), (0.5, 0, -1)], [(4, 0.25, 65504.0), (2, 1, 0)]], np.float16))


@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (37, 17)])
@pytest.mark.parametrize("pixel_type", ["half", "float"])
@pytest.mark.parametrize("compression", ["zip", "zips", "none"])
def test_reader_round_trips_reference_files(shape, pixel_type, compression):
    W, H = shape
    image, guides, s2, counts = _inputs(W, H, seed=W * 100 + H)
    for mask in (127, 3, 32, 0):
        kinds = []
        data = xa.encode(image, guides, s2, counts, mask, pixel_type, compression, 1024, scale=0.5, info=kinds)
        assert len(data) <= xa.capacity(W, H, pixel_type, compression, mask)
        back, info = exr.read(data)
        assert info["channel_names"] == [n for n, _ in xa.channel_list(mask, pixel_type)] and (info["width"], info["height"]) == (W, H)
        with np.errstate(all="ignore"):
            mean = (image / counts[..., None]).astype(F)
        assert np.array_equal(_bits(back), _bits(xr.convert(mean, 0.5, pixel_type)))      # scale acts on the radiance
        var = xa.variance_of_mean(image, s2, counts)
        source = {"Z": guides[..., 1], "N.X": guides[..., 2], "N.Y": guides[..., 3], "N.Z": guides[..., 4], "albedo.R": guides[..., 5], "albedo.G": guides[..., 6],
                  "albedo.B": guides[..., 7], "coverage": guides[..., 0], "transmittance": guides[..., 8], "variance.R": var[..., 0], "variance.G": var[..., 1],
                  "variance.B": var[..., 2], "samples": counts}
        for name, t in xa.channel_list(mask, pixel_type):
            if name in "RGB":
                continue
            got, v = info["channels"][name], source[name]
            if t == "half":
                assert got.dtype == np.float16 and np.array_equal(_bits(got), _bits(xr.convert(v, 1.0, "half"))), name      # and no scale on an AOV
                keep = ~np.isnan(v)
                assert np.array_equal(_bits(got)[keep], xr.half_bits_integer(_bits(v.astype(F))[keep])), name
            else:
                assert got.dtype == F and np.array_equal(_bits(got), np.where(np.isnan(v), np.uint32(0), _bits(v.astype(F)))), name      # the input's bits
        for blk, kind in zip(info["blocks"], kinds):
            assert blk["raw"] == (kind == "raw")
            if not blk["raw"]:
                lines = min(info["lines_per_block"], H - blk["y"])
                assert len(zlib.decompress(data[blk["offset"] + 8:blk["offset"] + 8 + blk["data_size"]])) == lines * W * xa.pixel_bytes(mask, pixel_type)
        if mask == 0:
            assert data == xr.encode(mean, pixel_type, compression, 1024, 0.5)


def test_variance_against_float64():
    """With u = 2^-24 the unit roundoff, D = S2 - S1^2 / n and Pe = S1^2 / n exact: the float32 chain is mean = (S1 / n)(1 + e1), prod = Pe (1 + e1)
    (1 + e2), d = (S2 - prod)(1 + e3), q = d / (n - 1) (1 + e4) (n - 1 is exact), v = max(0, q) / n (1 + e5), every |e| <= u.  S2 - prod differs
    from D by at most Pe (2 u + u^2); max(0, .) does not widen a difference.  So |v - v64| <= (|D| ((1 + u)^3 - 1) + Pe (2 u + u^2)(1 + u)^3) /
    (n (n - 1)) <= (4 u |D| + 3 u Pe) / (n (n - 1)) for values far from underflow, which these are."""
    rng = np.random.default_rng(5)
    N = 20000
    n = rng.integers(2, 200, N).astype(F)
    s1 = (rng.uniform(0.01, 500.0, (N, 3))).astype(F)
    s2 = (s1.astype(np.float64) ** 2 / n[:, None] * rng.uniform(0.98, 4.0, (N, 3))).astype(F)
    got = xa.variance_of_mean(s1, s2, n)
    assert got.dtype == F
    s1d, s2d, nd = s1.astype(np.float64), s2.astype(np.float64), n.astype(np.float64)[:, None]
    Pe = s1d * s1d / nd
    D = s2d - Pe
    want = np.maximum(0.0, D / (nd - 1.0)) / nd
    u = 2.0 ** -24
    bound = (4 * u * np.abs(D) + 3 * u * Pe) / (nd * (nd - 1.0))
    err = np.abs(got.astype(np.float64) - want)
    print("variance: largest error over its bound %.3f" % float((err / bound).max()))
    assert (err <= bound).all()
    assert (want > 0).mean() > 0.5 and (got == 0).sum() > 100     # both sides of the clamp are met
    # exactly 0: n < 2, and S2 < S1 mean
    for few in (0.0, 1.0, 1.5, np.nan):
        assert not xa.variance_of_mean(s1, s2, np.full(N, few, F)).any()
    low = (s1 * (s1 / n[:, None]).astype(F)).astype(F)
    below = np.nextafter(low, F(-np.inf)).astype(F)
    z = xa.variance_of_mean(s1, below, n)
    assert z.dtype == F and not z.any() and not np.signbit(z).any()
    assert not xa.variance_of_mean(s1, low, n).any()             # S2 == S1 mean: 0 too
    assert xa.variance_of_mean(F([[3.0, 3.0, 3.0]]), F([[6.0, 5.0, 4.5]]), F([2.0])).tolist() == [[0.75, 0.25, 0.0]]      # (S2 - 4.5) / 1 / 2
