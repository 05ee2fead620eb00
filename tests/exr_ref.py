"""The OpenEXR output restated in numpy (include/digital_earth_exr.h is the contract): the sample conversion, the front, the raw
block bytes, the reorder and the predictor, the zlib stream over deflate chunks — tests/png_ref.py's chunk coder by import, so the deflate is stated
once on the test side too —, the raw fallback, the offset table.  encode() gives the bytes the GPU must give."""
import struct
import zlib

import numpy as np

import png_ref

FRONT_FIXED = 313
DEFAULT_CHUNK = 32768
PIXEL_TYPES = {"half": 1, "float": 2}
COMPRESSIONS = {"none": 0, "zips": 2, "zip": 3}
LINES = {"none": 1, "zips": 1, "zip": 16}
F = np.float32


def convert(mean, scale=1.0, pixel_type="half"):
    """float32 means -> the stored samples: v = mean * scale in float32, a NaN +0; FLOAT the bits of v, HALF clip(v, +-65504) to nearest even."""
    with np.errstate(all="ignore"):
        v = (np.asarray(mean, F) * F(scale)).astype(F)
        v = np.where(np.isnan(v), F(0.0), v)
        if pixel_type == "float":
            return v.astype("<f4")
        return np.clip(v, F(-65504.0), F(65504.0)).astype("<f2")


def half_bits_integer(bits):
    """The header's integer statement of the HALF conversion on float32 bit patterns that are no NaN, written apart from numpy's cast."""
    out = []
    for x in (int(b) for b in np.asarray(bits, np.uint32).ravel()):
        s, a = (x >> 16) & 0x8000, x & 0x7fffffff
        if a >= 0x477fe000:
            h = 0x7bff
        elif a >= 0x38800000:
            h = (a + 0xfff + ((a >> 13) & 1) - 0x38000000) >> 13
        elif a <= 0x33000000:
            h = 0
        else:
            e, m = a >> 23, (a & 0x7fffff) | 0x800000
            k = 126 - e
            h, r, half = m >> k, m & ((1 << k) - 1), 1 << (k - 1)
            if r > half or (r == half and (h & 1)):
                h += 1
        out.append(s | h)
    return np.array(out, np.uint16).reshape(np.shape(bits))


def _attr(name, kind, value):
    return name + b"\0" + kind + b"\0" + struct.pack("<i", len(value)) + value


def front(W, H, pixel_type="half", compression="zip"):
    """Magic, version, the eight attributes, the closing byte: 313 bytes.  The offset table follows."""
    chlist = b"".join(n + b"\0" + struct.pack("<iB3xii", PIXEL_TYPES[pixel_type], 0, 1, 1) for n in (b"B", b"G", b"R")) + b"\0"
    box = struct.pack("<4i", 0, 0, W - 1, H - 1)
    out = (b"\x76\x2f\x31\x01\x02\x00\x00\x00" + _attr(b"channels", b"chlist", chlist) + _attr(b"compression", b"compression", bytes([COMPRESSIONS[compression]]))
           + _attr(b"dataWindow", b"box2i", box) + _attr(b"displayWindow", b"box2i", box) + _attr(b"lineOrder", b"lineOrder", b"\0")
           + _attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0)) + _attr(b"screenWindowCenter", b"v2f", struct.pack("<ff", 0.0, 0.0))
           + _attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")
    assert len(out) == FRONT_FIXED
    return out


def capacity(W, H, pixel_type="half", compression="zip"):
    nb = (H + LINES[compression] - 1) // LINES[compression]
    return FRONT_FIXED + 8 * nb + 8 * nb + H * W * 3 * (4 if pixel_type == "float" else 2)


def raw_block(samples):
    """(lines, W, 3) stored samples in R, G, B order -> r: per line all of B, then G, then R."""
    return np.ascontiguousarray(samples[:, :, ::-1].transpose(0, 2, 1)).tobytes()


def predict(r):
    r = np.frombuffer(r, np.uint8)
    t = np.concatenate((r[0::2], r[1::2])).astype(np.int32)
    p = t.copy()
    p[1:] = (t[1:] - t[:-1] + 128) & 255
    return p.astype(np.uint8)


def zip_payload(r, chunk_bytes=DEFAULT_CHUNK, info=None):
    p = predict(r)
    cuts = list(range(0, len(p), chunk_bytes))
    return (b"".join(png_ref.deflate_chunk(p[lo:lo + chunk_bytes], k == 0, k == len(cuts) - 1, info) for k, lo in enumerate(cuts))
            + struct.pack(">I", zlib.adler32(p.tobytes()) & 0xffffffff))


def encode(image, pixel_type="half", compression="zip", chunk_bytes=DEFAULT_CHUNK, scale=1.0, info=None):
    """The file the GPU writes for the (H, W, 3) float32 image, rows top-down, R, G, B.  info: a list that receives "raw" / "zip" per block."""
    image = np.asarray(image, F)
    H, W = image.shape[:2]
    samples = convert(image, scale, pixel_type)
    L = LINES[compression]
    blocks = []
    for y0 in range(0, H, L):
        r = raw_block(samples[y0:y0 + L])
        body = r
        if compression != "none":
            z = zip_payload(r, chunk_bytes)
            if len(z) < len(r):
                body = z
        if info is not None:
            info.append("raw" if body is r else "zip")
        blocks.append(struct.pack("<ii", y0, len(body)) + body)
    at = FRONT_FIXED + 8 * len(blocks)
    table = []
    for b in blocks:
        table.append(at)
        at += len(b)
    return front(W, H, pixel_type, compression) + struct.pack("<%dQ" % len(table), *table) + b"".join(blocks)
