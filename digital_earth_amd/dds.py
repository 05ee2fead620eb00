"""A dependency-free reader and writer for exactly the DDS files Renderer.fetch_ibl_dds() delivers (include/digital_earth_ibl.h): one cube map with
the DX10 header, R16G16B16A16_FLOAT or R32G32B32A32_FLOAT, L mip levels, face-major with each face followed by its levels, rows top first.

    write(levels, pixel_type="half") -> bytes      levels[l]: (6, e, e, 3) float32, e = E >> l; A = 1 is added
    read(data) -> (levels, info)                   levels[l]: (6, e, e, 4) float32; info: edge, levels, pixel_type

read() names what it refuses: anything that is not such a file."""
import struct

import numpy as np

HEADER_BYTES = 148
FORMATS = {"half": (10, 8, np.float16), "float": (2, 16, np.float32)}      # DXGI format, bytes per texel, the sample type


class DdsError(ValueError):
    pass


def half_bits(values):
    """float32 -> binary16 bits as the library converts (digital_earth_exr.h's HALF): NaN to +0, clamped to +-65504, nearest even."""
    v = np.asarray(values, np.float32)
    v = np.where(np.isnan(v), np.float32(0), np.clip(v, np.float32(-65504), np.float32(65504))).astype(np.float32)
    return v.astype(np.float16).view(np.uint16)


def header(edge, levels, pixel_type="half"):
    fmt, bpp, _ = FORMATS[pixel_type]
    w = [0] * 37
    w[0], w[1], w[2] = 0x20534444, 124, 0x0002100F
    w[3], w[4], w[5], w[7] = edge, edge, edge * bpp, levels
    w[19], w[20], w[21] = 32, 0x4, 0x30315844
    w[27], w[28] = 0x00401008, 0x0000FE00
    w[32], w[33], w[34], w[35] = fmt, 3, 0x4, 1
    return struct.pack("<37I", *w)


def write(levels, pixel_type="half"):
    if pixel_type not in FORMATS:
        raise DdsError("pixel_type must be 'half' or 'float'")
    levels = [np.asarray(v, np.float32) for v in levels]
    E = levels[0].shape[1]
    for l, v in enumerate(levels):
        if v.shape != (6, E >> l, E >> l, 3) or (E >> l) < 1:
            raise DdsError("level %d must have shape (6, %d, %d, 3)" % (l, E >> l, E >> l))
    parts = [header(E, len(levels), pixel_type)]
    for face in range(6):
        for v in levels:
            e = v.shape[1]
            rgba = np.ones((e, e, 4), np.float32)
            rgba[..., :3] = v[face]
            parts.append(half_bits(rgba).tobytes() if pixel_type == "half" else rgba.tobytes())
    return b"".join(parts)


def read(data):
    data = bytes(data)
    if len(data) < HEADER_BYTES:
        raise DdsError("shorter than a DDS header with its DX10 extension (148 bytes)")
    w = struct.unpack("<37I", data[:HEADER_BYTES])
    if w[0] != 0x20534444:
        raise DdsError("not a DDS file (magic)")
    if w[1] != 124 or w[19] != 32:
        raise DdsError("header sizes are not 124 and 32")
    if not (w[20] & 0x4) or w[21] != 0x30315844:
        raise DdsError("no DX10 header: only files with the DX10 extension are read")
    by_format = {v[0]: k for k, v in FORMATS.items()}
    if w[32] not in by_format:
        raise DdsError("DXGI format %d: only R16G16B16A16_FLOAT (10) and R32G32B32A32_FLOAT (2) are read" % w[32])
    if w[33] != 3 or not (w[34] & 0x4) or w[35] != 1 or (w[28] & 0xFE00) != 0xFE00:
        raise DdsError("not a single complete cube map (dimension, TEXTURECUBE, array size, caps2)")
    E, L = w[4], w[7]
    if w[3] != E or E < 1 or (E & (E - 1)):
        raise DdsError("height and width must be the same power of two")
    if L < 1 or (E >> (L - 1)) < 1:
        raise DdsError("mipMapCount %d does not fit edge %d" % (L, E))
    pixel_type = by_format[w[32]]
    _, bpp, dtype = FORMATS[pixel_type]
    want = HEADER_BYTES + 6 * sum((E >> l) ** 2 for l in range(L)) * bpp
    if len(data) != want:
        raise DdsError("%d bytes, the header asks for %d" % (len(data), want))
    levels = [np.empty((6, E >> l, E >> l, 4), np.float32) for l in range(L)]
    at = HEADER_BYTES
    for face in range(6):
        for l in range(L):
            e = E >> l
            n = e * e * bpp
            levels[l][face] = np.frombuffer(data, dtype, e * e * 4, at).reshape(e, e, 4).astype(np.float32)
            at += n
    return levels, dict(edge=E, levels=L, pixel_type=pixel_type)
