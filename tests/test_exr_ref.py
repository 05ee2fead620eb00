"""The OpenEXR output's restatement (tests/exr_ref.py) against independent statements, without a GPU: every file of the case list decodes through
digital_earth_amd.exr.read — written from the layout, inflating with zlib.decompress and its Adler check — to the expected samples bit for bit; the
offset table, the block sizes and the capacity hold; the HALF conversion equals numpy's cast on the edge values and its integer statement; one file
is written out by hand."""
import struct
import zlib

import numpy as np
import pytest

import exr_cases as xc
import exr_ref as xr
from digital_earth_amd import exr

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


@pytest.mark.parametrize("name", sorted(xc.CASES))
def test_file_decodes_to_the_expected_samples(name):
    image, pixel_type, compression, chunk, scale = xc.CASES[name]
    data, kinds = xc.encoded(name)
    H, W = image.shape[:2]
    got, info = exr.read(data)
    want = xr.convert(image, scale, pixel_type)
    assert got.dtype == want.dtype and got.shape == (H, W, 3) and np.array_equal(_bits(got), _bits(want))
    assert (info["width"], info["height"], info["pixel_type"], info["compression"], info["lines_per_block"]) == (W, H, pixel_type, compression, xr.LINES[compression])
    assert info["attributes"] == ["channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio", "screenWindowCenter", "screenWindowWidth"]
    L, bps = xr.LINES[compression], want.dtype.itemsize
    assert len(info["blocks"]) == (H + L - 1) // L == len(kinds)
    at = xr.FRONT_FIXED + 8 * len(kinds)
    for b, (blk, kind) in enumerate(zip(info["blocks"], kinds)):
        P = min(L, H - b * L) * W * 3 * bps
        assert blk["offset"] == at and struct.unpack_from("<i", data, at)[0] == blk["y"] == b * L      # the table points at each block's y0
        body = data[at + 8:at + 8 + blk["data_size"]]
        if kind == "zip":
            assert blk["data_size"] < P and not blk["raw"]
            p = zlib.decompress(body)                               # checks the Adler-32
            assert len(p) == P and exr.unpredict(p) == xr.raw_block(want[b * L:b * L + L])
            assert body[:2] == b"\x78\x01"
        else:
            assert blk["data_size"] == P and blk["raw"] and body == xr.raw_block(want[b * L:b * L + L])
        at += 8 + blk["data_size"]
    assert at == len(data) <= xr.capacity(W, H, pixel_type, compression)


def test_cases_reach_both_kinds_of_block():
    assert set(xc.encoded("random_bits_float")[1]) == {"raw"}
    assert set(xc.encoded("half_zero_float")[1]) == {"raw", "zip"}
    assert set(xc.encoded("8x1100_none")[1]) == {"raw"}
    assert "zip" in xc.encoded("700x33_half_1024")[1] and "zip" in xc.encoded("constant")[1]
    assert len(xc.encoded("3x17_zip")[1]) == 2 and len(xc.encoded("8x1100_zips")[1]) == 1100


def test_half_conversion_equals_numpys_cast_and_the_integer_statement():
    v = xc.HALF_EDGES
    got = xr.convert(v, 1.0, "half")
    with np.errstate(all="ignore"):
        clipped = np.clip(np.where(np.isnan(v), F(0), v), F(-65504), F(65504)).astype(np.float16)
    assert np.array_equal(_bits(got), _bits(clipped))
    table = dict(zip(v.view(np.uint32).tolist(), _bits(got).tolist()))
    b = lambda x: int(np.array(x, F).view(np.uint32))
    assert table[b(0.0)] == 0 and table[b(-0.0)] == 0x8000
    assert table[b(2.0 ** -24)] == 1 and table[b(2.0 ** -25)] == 0 and table[b(2.0 ** -24 * 1.5)] == 2      # the smallest, the tie to zero, the tie to even
    assert table[b(2.0 ** -14 - 2.0 ** -24)] == 0x03ff and table[b(2.0 ** -14)] == 0x0400
    assert table[b(1.0 + 2.0 ** -11)] == 0x3c00 and table[b(1.0 + 3.0 * 2.0 ** -11)] == 0x3c02           # ties both ways
    assert table[b(65504.0)] == table[b(65519.99)] == table[b(65520.0)] == table[b(1e30)] == table[b(np.inf)] == 0x7bff
    assert table[b(-np.inf)] == 0xfbff
    assert _bits(xr.convert(np.array([np.nan, -np.nan], F), 1.0, "half")).tolist() == [0, 0]
    assert _bits(xr.convert(np.array([np.nan], F), 1.0, "float")).tolist() == [0]
    # the header's integer statement on the edges and on random patterns of every exponent
    rng = np.random.default_rng(3)
    bits = np.concatenate((v.view(np.uint32), rng.integers(0, 1 << 32, 20000, dtype=np.uint64).astype(np.uint32),
                           (rng.integers(0x33000000 - 64, 0x38800000 + 64, 20000, dtype=np.uint64)).astype(np.uint32)))
    bits = bits[(bits & 0x7fffffff) <= 0x7f800000]
    assert np.array_equal(xr.half_bits_integer(bits), _bits(xr.convert(bits.view(F), 1.0, "half")))


def test_scale_is_one_float32_multiplication():
    img = xc.CASES["scale_half"][0]
    assert np.array_equal(_bits(xr.convert(img, 0.5, "float")), _bits((img * F(0.5)).astype(F)))
    assert np.array_equal(_bits(exr.read(xc.encoded("scale_3")[0])[0]), _bits((img * F(3.0)).astype(F)))


def test_a_file_written_out_by_hand():
    """2 x 2, HALF, NONE: row 0 = (1, 2, 3), (0.5, 0, -1); row 1 = (4, 0.25, 65504), (2, 1, 0) as R, G, B."""
    i32 = lambda v: struct.pack("<i", v)
    channel = lambda n: n + b"\0" + b"\x01\0\0\0" + b"\0" + b"\0\0\0" + b"\x01\0\0\0" + b"\x01\0\0\0"
    box = b"\0\0\0\0" + b"\0\0\0\0" + b"\x01\0\0\0" + b"\x01\0\0\0"
    front = (b"\x76\x2f\x31\x01" + b"\x02\0\0\0"
             + b"channels\0chlist\0" + b"\x37\0\0\0" + channel(b"B") + channel(b"G") + channel(b"R") + b"\0"
             + b"compression\0compression\0" + b"\x01\0\0\0" + b"\0"
             + b"dataWindow\0box2i\0" + b"\x10\0\0\0" + box
             + b"displayWindow\0box2i\0" + b"\x10\0\0\0" + box
             + b"lineOrder\0lineOrder\0" + b"\x01\0\0\0" + b"\0"
             + b"pixelAspectRatio\0float\0" + b"\x04\0\0\0" + b"\0\0\x80\x3f"
             + b"screenWindowCenter\0v2f\0" + b"\x08\0\0\0" + b"\0\0\0\0\0\0\0\0"
             + b"screenWindowWidth\0float\0" + b"\x04\0\0\0" + b"\0\0\x80\x3f"
             + b"\0")
    assert len(front) == 313
    table = struct.pack("<QQ", 329, 349)
    block0 = i32(0) + i32(12) + b"\x00\x42\x00\xbc" + b"\x00\x40\x00\x00" + b"\x00\x3c\x00\x38"      # B: 3, -1; G: 2, 0; R: 1, 0.5
    block1 = i32(1) + i32(12) + b"\xff\x7b\x00\x00" + b"\x00\x34\x00\x3c" + b"\x00\x44\x00\x40"      # B: 65504, 0; G: 0.25, 1; R: 4, 2
    want = front + table + block0 + block1
    image = np.array([[(1, 2, 3), (0.5, 0, -1)], [(4, 0.25, 70000.0), (2, 1, 0)]], F)               # 70000 clamps to 65504
    assert xr.encode(image, "half", "none") == want and len(want) == 369 == xr.capacity(2, 2, "half", "none")
    back, info = exr.read(want)
    assert np.array_equal(back, np.array([[(1, 2, 3), (0.5, 0, -1)], [(4, 0.25, 65504.0), (2, 1, 0)]], np.float16)) and info["compression"] == "none"


def test_reader_names_what_it_refuses():
    data = bytearray(xc.encoded("1x1")[0])
    for change, word in (((0, 0x77), "magic"), ((5, 0x02), "tiled"), ((5, 0x10), "multi-part"), ((5, 0x08), "deep")):
        bad = bytearray(data)
        bad[change[0]] = change[1]
        with pytest.raises(exr.ExrError, match=word):
            exr.read(bad)
    at = bytes(data).index(b"compression\0compression\0") + 24 + 4
    bad = bytearray(data); bad[at] = 4
    with pytest.raises(exr.ExrError, match="PIZ"):
        exr.read(bad)
    bad = bytearray(data); bad[bytes(data).index(b"B\0")] = ord("A")
    with pytest.raises(exr.ExrError, match="channels"):
        exr.read(bad)
    with pytest.raises(exr.ExrError):
        exr.read(bytes(data[:-1]))                                   # a block that passes the end
    bad = bytearray(xc.encoded("constant")[0]); bad[-1] ^= 0x40      # (its last block is compressed) the Adler-32 no longer holds
    with pytest.raises(zlib.error):
        exr.read(bad)
