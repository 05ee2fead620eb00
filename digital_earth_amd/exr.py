"""A minimal reader of the OpenEXR files this project's GPU encoder writes (include/digital_earth_exr.h): single-part scan-line files with the
channels B, G, R of one pixel type (HALF or FLOAT) and, beside them, any further channels of HALF or FLOAT type each (the AOV channels of
include/digital_earth_exr_aovs.h: a line holds every channel's samples in the channel list's order, which must be sorted by name as bytes),
compression NONE, ZIPS or ZIP, increasing line order, no subsampling.  Written from the file layout, not from the encoder: it is the tests' independent decoder and the user's way back in.  Inflate is zlib.decompress (which checks the
Adler-32); numpy only assembles the array.  Anything else — tiles, multi-part, deep data, UINT or subsampled channels, a channel list without B, G, R or out of order, other compressions — is
refused by name."""
import struct
import zlib

import numpy as np

MAGIC = b"\x76\x2f\x31\x01"
PIXEL_TYPES = {1: ("half", np.dtype("<f2")), 2: ("float", np.dtype("<f4"))}
COMPRESSIONS = {0: ("none", 1), 2: ("zips", 1), 3: ("zip", 16)}      # number -> (name, scan lines per block)
_REFUSED_COMPRESSIONS = {1: "RLE", 4: "PIZ", 5: "PXR24", 6: "B44", 7: "B44A", 8: "DWAA", 9: "DWAB"}


class ExrError(ValueError):
    """The file is not one this reader takes; the message names what it met."""


def _cstring(data, at):
    end = data.find(b"\0", at)
    if end < 0 or end - at > 255:
        raise ExrError("an unterminated name in the header")
    return data[at:end], end + 1


def _attributes(data, at):
    """The header's attributes from `at` on: ({name: (type, value bytes)}, the names in file order, the offset behind the header's closing byte)."""
    attrs, order = {}, []
    while True:
        if at >= len(data):
            raise ExrError("the header does not end")
        if data[at] == 0:
            return attrs, order, at + 1
        name, at = _cstring(data, at)
        kind, at = _cstring(data, at)
        if at + 4 > len(data):
            raise ExrError("the header does not end")
        size, = struct.unpack_from("<i", data, at)
        at += 4
        if size < 0 or at + size > len(data):
            raise ExrError("attribute %r passes the end of the file" % name.decode("latin-1"))
        attrs[name.decode("latin-1")] = (kind.decode("latin-1"), data[at:at + size])
        order.append(name.decode("latin-1"))
        at += size


def _channels(value):
    out, at = [], 0
    while True:
        if at >= len(value):
            raise ExrError("the channel list does not end")
        if value[at] == 0:
            if at + 1 != len(value):
                raise ExrError("bytes behind the channel list")
            return out
        name, at = _cstring(value, at)
        if at + 16 > len(value):
            raise ExrError("the channel list does not end")
        ptype, plinear, xs, ys = struct.unpack_from("<iB3xii", value, at)
        at += 16
        out.append((name.decode("latin-1"), ptype, plinear, xs, ys))


def unpredict(p):
    """The ZIP payload's inverse: the predictor undone (a running sum from p[0], 128 taken off each step), then the two halves interleaved again."""
    p = np.frombuffer(p, np.uint8)
    n = len(p)
    if n == 0:
        return b""
    steps = p.astype(np.int64)
    steps[1:] -= 128
    t = (np.cumsum(steps) & 255).astype(np.uint8)
    h = (n + 1) // 2
    r = np.empty(n, np.uint8)
    r[0::2] = t[:h]
    r[1::2] = t[h:]
    return r.tobytes()


def read(data):
    """An OpenEXR file of this encoder's kind -> (array [H][W][3] float16 | float32 in R, G, B order, rows top-down; info).  info: width, height,
    pixel_type ("half" | "float": of B, G, R), compression ("none" | "zips" | "zip"), lines_per_block, blocks (per block: y, offset, data_size, raw),
    attributes (the header's names in file order), channel_names (in file order), channel_types (name -> "half" | "float") and channels: every
    channel of the file, B, G and R included, as name -> array [H][W] of its own type.  Raises ExrError naming what it refuses."""
    data = bytes(data)
    if len(data) < 8 or data[:4] != MAGIC:
        raise ExrError("not an OpenEXR file: the magic number is missing")
    version, = struct.unpack_from("<I", data, 4)
    if version & 0xff != 2:
        raise ExrError("OpenEXR version %d, not 2" % (version & 0xff))
    for bit, what in ((0x200, "a tiled file"), (0x400, "long names"), (0x800, "deep data"), (0x1000, "a multi-part file")):
        if version & bit:
            raise ExrError("%s is not supported" % what)
    attrs, order, at = _attributes(data, 8)

    def need(name, kind, size):
        if name not in attrs:
            raise ExrError("the required attribute %r is missing" % name)
        k, v = attrs[name]
        if k != kind or len(v) != size:
            raise ExrError("attribute %r is a %s of %d bytes, not a %s of %d" % (name, k, len(v), kind, size))
        return v
    if "channels" not in attrs or attrs["channels"][0] != "chlist":
        raise ExrError("the required attribute 'channels' is missing")
    chans = _channels(attrs["channels"][1])
    names = [c[0] for c in chans]
    if not {"B", "G", "R"} <= set(names):
        raise ExrError("channels %s hold no B, G, R" % ", ".join(names))
    if len(set(names)) != len(names) or [n.encode("latin-1") for n in names] != sorted(n.encode("latin-1") for n in names):
        raise ExrError("channels %s are not sorted by name" % ", ".join(names))
    colour = [c for c in chans if c[0] in ("B", "G", "R")]
    if len({c[1] for c in colour}) != 1 or any(c[1] not in PIXEL_TYPES for c in chans):
        raise ExrError("the channels' pixel types %s: B, G, R must share one, and every channel be HALF or FLOAT" % [c[1] for c in chans])
    if any(c[3] != 1 or c[4] != 1 for c in chans):
        raise ExrError("subsampled channels are not supported")
    type_name, dtype = PIXEL_TYPES[colour[0][1]]
    dtypes = [PIXEL_TYPES[c[1]][1] for c in chans]
    pixel_bytes = sum(d.itemsize for d in dtypes)
    comp = need("compression", "compression", 1)[0]
    if comp not in COMPRESSIONS:
        raise ExrError("compression %s is not supported" % _REFUSED_COMPRESSIONS.get(comp, comp))
    comp_name, L = COMPRESSIONS[comp]
    x0, y0, x1, y1 = struct.unpack("<4i", need("dataWindow", "box2i", 16))
    if struct.unpack("<4i", need("displayWindow", "box2i", 16)) != (x0, y0, x1, y1) or (x0, y0) != (0, 0) or x1 < 0 or y1 < 0:
        raise ExrError("a data window other than the display window from (0, 0) is not supported")
    if need("lineOrder", "lineOrder", 1)[0] != 0:
        raise ExrError("a line order other than increasing y is not supported")
    for name, kind, size in (("pixelAspectRatio", "float", 4), ("screenWindowCenter", "v2f", 8), ("screenWindowWidth", "float", 4)):
        need(name, kind, size)
    W, H = x1 + 1, y1 + 1
    nb = (H + L - 1) // L
    if at + 8 * nb > len(data):
        raise ExrError("the offset table passes the end of the file")
    offsets = struct.unpack_from("<%dQ" % nb, data, at)
    out = np.empty((H, W, 3), dtype)
    planes = {n: np.empty((H, W), d) for n, d in zip(names, dtypes)}
    blocks = []
    for b, off in enumerate(offsets):
        if off + 8 > len(data):
            raise ExrError("block %d lies behind the end of the file" % b)
        y, size = struct.unpack_from("<ii", data, off)
        lines = min(L, H - b * L)
        P = lines * W * pixel_bytes
        if y != b * L:
            raise ExrError("the offset table's entry %d points at a block of line %d" % (b, y))
        if size < 0 or size > P or off + 8 + size > len(data):
            raise ExrError("block %d has dataSize %d for %d raw bytes" % (b, size, P))
        body = data[off + 8:off + 8 + size]
        raw = size == P
        if not raw:
            if comp == 0:
                raise ExrError("block %d of an uncompressed file is short" % b)
            body = unpredict(zlib.decompress(body))
            if len(body) != P:
                raise ExrError("block %d inflates to %d bytes, not %d" % (b, len(body), P))
        rows = np.frombuffer(body, np.uint8).reshape(lines, W * pixel_bytes)      # per line: every channel's W samples, in the list's order
        at = 0
        for n, d in zip(names, dtypes):
            planes[n][b * L:b * L + lines] = np.ascontiguousarray(rows[:, at:at + W * d.itemsize]).view(d)
            at += W * d.itemsize
        blocks.append(dict(y=y, offset=off, data_size=size, raw=raw))
    for k, n in enumerate("RGB"):
        out[:, :, k] = planes[n]
    return out, dict(width=W, height=H, pixel_type=type_name, compression=comp_name, lines_per_block=L, blocks=blocks, attributes=order,
                     channel_names=names, channel_types={n: PIXEL_TYPES[c[1]][0] for n, c in zip(names, chans)}, channels=planes)
