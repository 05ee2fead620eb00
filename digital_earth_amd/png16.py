"""A minimal writer of 16-bit RGB PNG files with a `cICP` chunk (PNG, third edition: coding-independent code points, ITU-T H.273) — what
EarthViewer.save writes while the HDR display output is on.  Built on zlib and struct alone: the image writer the 8-bit screenshots go through has no
16-bit RGB mode.  Every row is stored with filter type 0; the samples are big-endian, as PNG asks."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
CICP_PRIMARIES = {"rec709": 1, "p3d65": 12, "rec2020": 9}
CICP_TRANSFER = {"linear": 8, "pq": 16, "hlg": 18}


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def cicp_of(gamut, transfer):
    """(colour primaries, transfer function, matrix coefficients = 0: RGB, full range = 1) of a setting of Renderer.set_hdr_output."""
    return (CICP_PRIMARIES[gamut], CICP_TRANSFER[transfer], 0, 1)


def to_rgb16(held):
    """A held picture as (H, W, 3) uint16 rows top-down, on the host, without a new display: uint16 (H, W, 3) as it is; RGB10A2 uint32 (H, W) with
    every 10-bit code c widened to (c << 6) | (c >> 4) (0 stays 0, 1023 becomes 65535, alpha dropped); uint8 (H, W, 3 | 4) times 257; a float signal
    (W, H, 3), row 0 at the bottom, clipped to [0, 1] (NaN to 0), scaled by 65535 and rounded — the ROUND formula of the GPU pack in float32."""
    a = np.asarray(held)
    if a.dtype == np.uint16 and a.ndim == 3 and a.shape[2] == 3:
        return a
    if a.dtype == np.uint32 and a.ndim == 2:
        c = np.stack([a & 1023, (a >> 10) & 1023, (a >> 20) & 1023], axis=-1)
        return ((c << 6) | (c >> 4)).astype(np.uint16)
    if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] in (3, 4):
        return a[..., :3].astype(np.uint16) * np.uint16(257)
    if a.dtype == np.float32 and a.ndim == 3 and a.shape[2] == 3:
        with np.errstate(invalid="ignore"):
            cl = np.where(a > 0, np.where(a < 1, a, np.float32(1)), np.float32(0)).astype(np.float32)
        q = (cl * np.float32(65535.0) + np.float32(0.5)).astype(np.int32).astype(np.uint16)
        return np.ascontiguousarray(q.transpose(1, 0, 2)[::-1])
    raise ValueError("not a picture this writer knows: %s %s" % (a.dtype, a.shape))


def encode_png16(px, cicp, level=6):
    """px: (H, W, 3) uint16, rows top-down; cicp: four bytes.  Returns the file's bytes: IHDR (bit depth 16, colour type 2), cICP ahead of IDAT, IEND."""
    px = np.asarray(px)
    if px.dtype != np.uint16 or px.ndim != 3 or px.shape[2] != 3:
        raise ValueError("px must be (H, W, 3) uint16")
    h, w = px.shape[:2]
    rows = np.zeros((h, 1 + w * 6), np.uint8)                  # column 0: the filter type of every row, 0
    rows[:, 1:] = px.astype(">u2").view(np.uint8).reshape(h, w * 6)
    return b"".join((SIGNATURE, _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0)), _chunk(b"cICP", struct.pack("BBBB", *cicp)),
                     _chunk(b"IDAT", zlib.compress(rows.tobytes(), level)), _chunk(b"IEND", b"")))


def write_png16(path, px, cicp):
    with open(path, "wb") as f:
        f.write(encode_png16(px, cicp))
