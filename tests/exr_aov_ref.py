"""The EXR output's AOV channels restated in numpy (include/digital_earth_exr_aovs.h is the contract): the channels of a mask and
their order — Python's sorted() on the encoded names —, the front with that channel list, the variance of the mean in float32 at every step, the
lines of mixed-type planes, the capacity and the limit.  The conversion, the predictor, the zlib stream and the chunk coder are tests/exr_ref.py's
and tests/png_ref.py's, by import.  encode() gives the bytes the GPU must give."""
import struct

import numpy as np

import exr_ref as xr

F = np.float32
BITS = {"depth": 1, "normal": 2, "albedo": 4, "coverage": 8, "transmittance": 16, "variance": 32, "samples": 64}
ALL = 127
MAX_RAW = 1 << 27
# name -> (the group's bit, 0: always there; always FLOAT; where the sample comes from: a guide's index in fetch_guides' order, or a word)
CHANNELS = {
    "R": (0, False, ("image", 0)), "G": (0, False, ("image", 1)), "B": (0, False, ("image", 2)),
    "Z": (1, True, ("guide", 1)),
    "N.X": (2, False, ("guide", 2)), "N.Y": (2, False, ("guide", 3)), "N.Z": (2, False, ("guide", 4)),
    "albedo.R": (4, False, ("guide", 5)), "albedo.G": (4, False, ("guide", 6)), "albedo.B": (4, False, ("guide", 7)),
    "coverage": (8, False, ("guide", 0)),
    "transmittance": (16, False, ("guide", 8)),
    "variance.R": (32, True, ("variance", 0)), "variance.G": (32, True, ("variance", 1)), "variance.B": (32, True, ("variance", 2)),
    "samples": (64, True, ("samples", 0)),
}


def channel_list(mask, pixel_type="half"):
    """[(name, "half" | "float")] of a mask in the file's order: sorted by name as bytes."""
    names = sorted(n.encode("ascii") for n, (bit, _, _) in CHANNELS.items() if not bit or mask & bit)
    return [(n.decode("ascii"), "float" if CHANNELS[n.decode("ascii")][1] else pixel_type) for n in names]


def pixel_bytes(mask, pixel_type="half"):
    return sum(4 if t == "float" else 2 for _, t in channel_list(mask, pixel_type))


def within_limit(W, H, mask, pixel_type="half"):
    return H * W * pixel_bytes(mask, pixel_type) <= MAX_RAW


def front(W, H, pixel_type="half", compression="zip", mask=0):
    """Magic, version, the eight attributes with the mask's channel list, the closing byte.  The offset table follows."""
    chlist = b"".join(n.encode("ascii") + b"\0" + struct.pack("<iB3xii", xr.PIXEL_TYPES[t], 0, 1, 1) for n, t in channel_list(mask, pixel_type)) + b"\0"
    box = struct.pack("<4i", 0, 0, W - 1, H - 1)
    return (b"\x76\x2f\x31\x01\x02\x00\x00\x00" + xr._attr(b"channels", b"chlist", chlist) + xr._attr(b"compression", b"compression", bytes([xr.COMPRESSIONS[compression]]))
            + xr._attr(b"dataWindow", b"box2i", box) + xr._attr(b"displayWindow", b"box2i", box) + xr._attr(b"lineOrder", b"lineOrder", b"\0")
            + xr._attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0)) + xr._attr(b"screenWindowCenter", b"v2f", struct.pack("<ff", 0.0, 0.0))
            + xr._attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0)) + b"\0")


def capacity(W, H, pixel_type="half", compression="zip", mask=0):
    nb = (H + xr.LINES[compression] - 1) // xr.LINES[compression]
    return len(front(W, H, pixel_type, compression, mask)) + 8 * nb + 8 * nb + H * W * pixel_bytes(mask, pixel_type)


def variance_of_mean(s1, s2, n):
    """THE VARIANCE: float32 at every step.  mean = S1 / n; prod = S1 * mean; d = S2 - prod; q = d / (n - 1); sv = q if q > 0 else 0; sv / n;
    0 where n < 2.  s1, s2 (..., 3), n (...)."""
    s1, s2 = np.asarray(s1, F), np.asarray(s2, F)
    n = np.asarray(n, F)[..., None]
    with np.errstate(all="ignore"):
        mean = (s1 / n).astype(F)
        prod = (s1 * mean).astype(F)
        d = (s2 - prod).astype(F)
        q = (d / (n - F(1.0)).astype(F)).astype(F)
        sv = np.where(q > F(0.0), q, F(0.0)).astype(F)
        v = (sv / n).astype(F)
    return np.where(n >= F(2.0), v, F(0.0)).astype(F)


def float_sample(v):
    """A FLOAT AOV channel: the 32 bits, a NaN +0."""
    v = np.asarray(v, F)
    return np.where(np.isnan(v), F(0.0), v).astype("<f4")


def stored_planes(image, guides=None, s2=None, counts=None, mask=0, pixel_type="half", scale=1.0):
    """name -> the stored samples (H, W) of every channel of the mask, in the file's order (a dict keeps it).  image (H, W, 3) is read as the sums,
    counts (H, W) as the divisor (None: 1) of B, G, R too; guides (H, W, 9) in fetch_guides' order; s2 (H, W, 3)."""
    image = np.asarray(image, F)
    H, W = image.shape[:2]
    n = np.ones((H, W), F) if counts is None else np.asarray(counts, F)
    with np.errstate(all="ignore"):
        mean = (image / n[..., None]).astype(F)
    out = {}
    for name, t in channel_list(mask, pixel_type):
        kind, k = CHANNELS[name][2]
        if kind == "image":
            out[name] = xr.convert(mean[..., k], scale, pixel_type)
            continue
        v = {"guide": lambda: np.asarray(guides, F)[..., k], "variance": lambda: variance_of_mean(image, s2, n)[..., k], "samples": lambda: n}[kind]()
        out[name] = float_sample(v) if t == "float" else xr.convert(v, 1.0, pixel_type)
    return out


def raw_block(planes, y0, lines):
    """r of the lines y0 ... y0 + lines - 1: for each line, every channel's W samples in the file's order."""
    return b"".join(np.ascontiguousarray(p[y]).tobytes() for y in range(y0, y0 + lines) for p in planes.values())


def encode(image, guides=None, s2=None, counts=None, mask=0, pixel_type="half", compression="zip", chunk_bytes=xr.DEFAULT_CHUNK, scale=1.0, info=None):
    """The file the GPU writes.  info: a list that receives "raw" / "zip" per block."""
    image = np.asarray(image, F)
    H, W = image.shape[:2]
    planes = stored_planes(image, guides, s2, counts, mask, pixel_type, scale)
    L = xr.LINES[compression]
    blocks = []
    for y0 in range(0, H, L):
        r = raw_block(planes, y0, min(L, H - y0))
        body = r
        if compression != "none":
            z = xr.zip_payload(r, chunk_bytes)
            if len(z) < len(r):
                body = z
        if info is not None:
            info.append("raw" if body is r else "zip")
        blocks.append(struct.pack("<ii", y0, len(body)) + body)
    head = front(W, H, pixel_type, compression, mask)
    at = len(head) + 8 * len(blocks)
    table = []
    for b in blocks:
        table.append(at)
        at += len(b)
    return head + struct.pack("<%dQ" % len(table), *table) + b"".join(blocks)
