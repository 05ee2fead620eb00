"""A dependency-free reader and writer of Radiance picture files (.hdr) as this project's GPU encoder writes them (include/digital_earth_rgbe.h):
FORMAT=32-bit_rle_rgbe, orientation -Y H +X W, rows flat or new-style run-length coded.  Written from the file layout, not from the encoder: it is
the tests' decoder and the user's way back in.  Anything else — XYZE, another orientation, old-style run-length coding — is refused by name.

TWO DECODING CONVENTIONS.  A pixel's bytes q_R q_G q_B E (E > 0) stand for the interval [q, q + 1) 2^(E - 136) under Radiance's own float2rgbe, which
truncates.  read(..., half_step=False) returns its lower end, q 2^(E - 136) — what stb_image, three.js and most importers return: exact for values
an encoder ROUNDED (set_rgbe(rounding="round"): |error| <= 1/2 step), biased low by half a step on average for a truncating encoder.
read(..., half_step=True) returns (q + 0.5) 2^(E - 136), Radiance's own rgbe2float: the centre of a truncating encoder's interval (rounding="trunc",
the default: |error| <= 1/2 step).  E == 0 is black under both.  Divide by info["exposure"] to come back to radiance where the file carries one.

write() is the host's encoder: the same file for the same settings, slowly."""
import re

import numpy as np

PRIMARIES_709 = b"0.64 0.33 0.3 0.6 0.15 0.06 0.3127 0.329"
MAX_VALUE = float(255 * 2.0 ** 119)


class RgbeError(ValueError):
    """The file is not one this reader takes; the message names what it met."""


def _bytes_of(source):
    if isinstance(source, (bytes, bytearray, memoryview)):
        return bytes(source)
    with open(source, "rb") as f:
        return f.read()


def parse_header(data):
    """(info, offset of the first row): info has width, height, format, exposure (the product of the EXPOSURE lines, 1.0 without one), primaries
    (eight floats or None) and lines, the header's lines as bytes."""
    if not data.startswith(b"#?"):
        raise RgbeError("no #? signature")
    end = data.find(b"\n\n")
    if end < 0:
        raise RgbeError("the header does not end")
    lines = data[:end].split(b"\n")
    res_end = data.find(b"\n", end + 2)
    if res_end < 0:
        raise RgbeError("no resolution line")
    res = data[end + 2:res_end]
    m = re.fullmatch(rb"-Y (\d+) \+X (\d+)", res)
    if not m:
        raise RgbeError("orientation %r: only -Y H +X W is read" % res.decode("latin-1"))
    info = dict(height=int(m.group(1)), width=int(m.group(2)), format=None, exposure=1.0, primaries=None, lines=lines)
    for line in lines[1:]:
        if line.startswith(b"FORMAT="):
            info["format"] = line[7:].decode("latin-1")
        elif line.startswith(b"EXPOSURE="):
            info["exposure"] *= float(line[9:])
        elif line.startswith(b"PRIMARIES="):
            info["primaries"] = tuple(float(x) for x in line[10:].split())
    if info["format"] != "32-bit_rle_rgbe":
        raise RgbeError("FORMAT=%s: only 32-bit_rle_rgbe is read" % info["format"])
    return info, res_end + 1


def decode(source):
    """The file's pixels as they are stored: ((H, W, 4) uint8 in R, G, B, E order, info).  info["rows"] says how each row was coded, "rle" or "flat"."""
    data = _bytes_of(source)
    info, at = parse_header(data)
    W, H = info["width"], info["height"]
    out = np.zeros((H, W, 4), np.uint8)
    rows = []
    for y in range(H):
        if 8 <= W <= 32767 and data[at:at + 2] == b"\x02\x02" and at + 4 <= len(data) and not data[at + 2] & 0x80:
            if (data[at + 2] << 8 | data[at + 3]) != W:
                raise RgbeError("row %d: a scanline of another width" % y)
            at += 4
            for c in range(4):
                x = 0
                while x < W:
                    if at >= len(data):
                        raise RgbeError("row %d: the file ends inside a plane" % y)
                    n = data[at]
                    if n > 128:
                        n -= 128
                        if x + n > W or at + 2 > len(data):
                            raise RgbeError("row %d: a run crosses the plane's end" % y)
                        out[y, x:x + n, c] = data[at + 1]
                        at += 2
                    else:
                        if n == 0 or x + n > W or at + 1 + n > len(data):
                            raise RgbeError("row %d: a literal packet of %d bytes at column %d" % (y, n, x))
                        out[y, x:x + n, c] = np.frombuffer(data, np.uint8, n, at + 1)
                        at += 1 + n
                    x += n
            rows.append("rle")
        else:
            if at + 4 * W > len(data):
                raise RgbeError("row %d: the file ends inside a flat row" % y)
            row = np.frombuffer(data, np.uint8, 4 * W, at).reshape(W, 4)
            if W >= 8 and W <= 32767 and (row[:, :3] == 1).all(axis=1).any():
                raise RgbeError("row %d: old-style run-length coding is not read" % y)
            out[y] = row
            at += 4 * W
            rows.append("flat")
    if at != len(data):
        raise RgbeError("%d bytes behind the last row" % (len(data) - at))
    info["rows"] = rows
    return out, info


def to_float(pixels, half_step=False):
    """(..., 4) uint8 R, G, B, E -> (..., 3) float32: q 2^(E - 136), or (q + 0.5) 2^(E - 136) with half_step; black where E == 0.  Exact in float32."""
    pixels = np.asarray(pixels, np.uint8)
    q = pixels[..., :3].astype(np.float64) + (0.5 if half_step else 0.0)
    e = pixels[..., 3:4].astype(np.int32)
    value = np.ldexp(q, e - 136)
    return np.where(e == 0, 0.0, value).astype(np.float32)


def read(source, half_step=False):
    """A .hdr file (a path, or its bytes) -> ((H, W, 3) float32 rows top-down in R, G, B order, info).  The two conventions: the module's docstring."""
    pixels, info = decode(source)
    return to_float(pixels, half_step), info


def _encode_pixels(image, rounding):
    v = np.asarray(image, np.float32).astype(np.float64)
    v = np.where(np.isnan(v) | (v < 0), 0.0, np.minimum(v, MAX_VALUE))
    m = v.max(axis=-1)
    _, e = np.frexp(m)
    scaled = np.ldexp(v, (8 - e)[..., None])
    q = np.floor(scaled + (0.5 if rounding == "round" else 0.0))
    up = q.max(axis=-1) >= 256
    if up.any():
        e = e + up
        q = np.where(up[..., None], np.floor(np.ldexp(v, (8 - e)[..., None]) + 0.5), q)
    out = np.zeros(v.shape[:-1] + (4,), np.uint8)
    out[..., :3] = np.minimum(q, 255).astype(np.uint8)
    out[..., 3] = np.clip(e + 128, 0, 255).astype(np.uint8)
    out[m < np.float64(np.float32(1e-32))] = 0
    return out


def _encode_plane(p):
    """One plane of a row: runs of four and more equal bytes as packets of at most 127, what lies between as literal packets of at most 128."""
    out, lit, W, i = bytearray(), bytearray(), len(p), 0

    def flush():
        for k in range(0, len(lit), 128):
            out.append(min(128, len(lit) - k))
            out.extend(lit[k:k + 128])
        del lit[:]
    while i < W:
        j = i
        while j < W and p[j] == p[i]:
            j += 1
        if j - i >= 4:
            flush()
            for k in range(i, j, 127):
                out.extend((128 + min(127, j - k), p[i]))
        else:
            lit.extend(p[i:j])
        i = j
    flush()
    return bytes(out)


def header(width, height, exposure=1.0):
    text = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\nPRIMARIES=" + PRIMARIES_709 + b"\n"
    if np.float32(exposure) != np.float32(1.0):
        text += b"EXPOSURE=" + ("%.9g" % float(np.float32(exposure))).encode() + b"\n"
    return text + b"\n-Y %d +X %d\n" % (height, width)


def write(path, image, rle=True, rounding="trunc", scale=1.0):
    """image (H, W, 3) float -> a .hdr file at `path` (None: nothing is written); returns its bytes.  scale is multiplied into the samples in float32
    and written as EXPOSURE; rounding "trunc" or "round"; rle=False: flat rows."""
    if rounding not in ("trunc", "round"):
        raise ValueError("rounding must be \"trunc\" or \"round\"")
    image = np.asarray(image, np.float32)
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("image must have shape (H, W, 3)")
    H, W = image.shape[:2]
    pixels = _encode_pixels(image * np.float32(scale), rounding)
    parts = [header(W, H, scale)]
    if rle and 8 <= W <= 32767:
        for y in range(H):
            parts.append(bytes((2, 2, W >> 8, W & 255)))
            for c in range(4):
                parts.append(_encode_plane(pixels[y, :, c].tobytes()))
    else:
        parts.append(pixels.tobytes())
    data = b"".join(parts)
    if path is not None:
        with open(path, "wb") as f:
            f.write(data)
    return data
