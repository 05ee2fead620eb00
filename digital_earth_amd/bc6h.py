"""BC6H_UF16 for exactly the files Renderer.fetch_ibl_bc6h_dds() delivers (include/digital_earth_ibl_bc6h.h), numpy only.

    decode_blocks(data, w, h) -> (h, w, 3) uint16      half bits of a w x h image stored as ceil(w / 4) ceil(h / 4) blocks, rows of blocks top first
    encode_blocks(half, quality) -> bytes              the header's encoder on an (h, w, 3) image of half integers 0 ... 0x7BFF, any w, h >= 1
    write(levels, quality=0) -> bytes                  levels[l]: (6, e, e, 3) float32 or uint16 half bits, e = E >> l
    read(data) -> (levels, info)                       levels[l]: (6, e, e, 3) uint16 half bits; info: edge, levels

All 14 modes are decoded; the tables below (field layouts, partitions, anchors) are written from the format's own tables, not taken from the library's
csrc/bc6h_tables.h — tests/test_ibl_bc6h_abi.py holds the two against each other.  read() names what it refuses: anything that is not such a file."""
import struct

import numpy as np

from .dds import DdsError, half_bits

HEADER_BYTES = 148
DXGI_BC6H_UF16 = 95
HALF_MAX = 0x7BFF

# mode number -> (mode bits' value, their count, endpoint precision, delta bits of R G B (0: the ends are direct), regions)
MODES = {1: (0, 2, 10, (5, 5, 5), 2), 2: (1, 2, 7, (6, 6, 6), 2), 3: (2, 5, 11, (5, 4, 4), 2), 4: (6, 5, 11, (4, 5, 4), 2), 5: (10, 5, 11, (4, 4, 5), 2),
         6: (14, 5, 9, (5, 5, 5), 2), 7: (18, 5, 8, (6, 5, 5), 2), 8: (22, 5, 8, (5, 6, 5), 2), 9: (26, 5, 8, (5, 5, 6), 2), 10: (30, 5, 6, (0, 0, 0), 2),
         11: (3, 5, 10, (0, 0, 0), 1), 12: (7, 5, 11, (9, 9, 9), 1), 13: (11, 5, 12, (8, 8, 8), 1), 14: (15, 5, 16, (4, 4, 4), 1)}
RESERVED = (19, 23, 27, 31)
# The bits behind the mode bits, in file order.  W, X: the ends of region 0; Y, Z: of region 1; D: the partition.  "a-b": bits a ... b, in that order.
LAYOUTS = {
    1: "GY:4 BY:4 BZ:4 RW:0-9 GW:0-9 BW:0-9 RX:0-4 GZ:4 GY:0-3 GX:0-4 BZ:0 GZ:0-3 BX:0-4 BZ:1 BY:0-3 RY:0-4 BZ:2 RZ:0-4 BZ:3 D:0-4",
    2: "GY:5 GZ:4 GZ:5 RW:0-6 BZ:0 BZ:1 BY:4 GW:0-6 BY:5 BZ:2 GY:4 BW:0-6 BZ:3 BZ:5 BZ:4 RX:0-5 GY:0-3 GX:0-5 GZ:0-3 BX:0-5 BY:0-3 RY:0-5 RZ:0-5 D:0-4",
    3: "RW:0-9 GW:0-9 BW:0-9 RX:0-4 RW:10 GY:0-3 GX:0-3 GW:10 BZ:0 GZ:0-3 BX:0-3 BW:10 BZ:1 BY:0-3 RY:0-4 BZ:2 RZ:0-4 BZ:3 D:0-4",
    4: "RW:0-9 GW:0-9 BW:0-9 RX:0-3 RW:10 GZ:4 GY:0-3 GX:0-4 GW:10 GZ:0-3 BX:0-3 BW:10 BZ:1 BY:0-3 RY:0-3 BZ:0 BZ:2 RZ:0-3 GY:4 BZ:3 D:0-4",
    5: "RW:0-9 GW:0-9 BW:0-9 RX:0-3 RW:10 BY:4 GY:0-3 GX:0-3 GW:10 BZ:0 GZ:0-3 BX:0-4 BW:10 BY:0-3 RY:0-3 BZ:1 BZ:2 RZ:0-3 BZ:4 BZ:3 D:0-4",
    6: "RW:0-8 BY:4 GW:0-8 GY:4 BW:0-8 BZ:4 RX:0-4 GZ:4 GY:0-3 GX:0-4 BZ:0 GZ:0-3 BX:0-4 BZ:1 BY:0-3 RY:0-4 BZ:2 RZ:0-4 BZ:3 D:0-4",
    7: "RW:0-7 GZ:4 BY:4 GW:0-7 BZ:2 GY:4 BW:0-7 BZ:3 BZ:4 RX:0-5 GY:0-3 GX:0-4 BZ:0 GZ:0-3 BX:0-4 BZ:1 BY:0-3 RY:0-5 RZ:0-5 D:0-4",
    8: "RW:0-7 BZ:0 BY:4 GW:0-7 GY:5 GY:4 BW:0-7 GZ:5 BZ:4 RX:0-4 GZ:4 GY:0-3 GX:0-5 GZ:0-3 BX:0-4 BZ:1 BY:0-3 RY:0-4 BZ:2 RZ:0-4 BZ:3 D:0-4",
    9: "RW:0-7 BZ:1 BY:4 GW:0-7 BY:5 GY:4 BW:0-7 BZ:5 BZ:4 RX:0-4 GZ:4 GY:0-3 GX:0-4 BZ:0 GZ:0-3 BX:0-5 BY:0-3 RY:0-4 BZ:2 RZ:0-4 BZ:3 D:0-4",
    10: "RW:0-5 GZ:4 BZ:0 BZ:1 BY:4 GW:0-5 GY:5 BY:5 BZ:2 GY:4 BW:0-5 GZ:5 BZ:3 BZ:5 BZ:4 RX:0-5 GY:0-3 GX:0-5 GZ:0-3 BX:0-5 BY:0-3 RY:0-5 RZ:0-5 D:0-4",
    11: "RW:0-9 GW:0-9 BW:0-9 RX:0-9 GX:0-9 BX:0-9",
    12: "RW:0-9 GW:0-9 BW:0-9 RX:0-8 RW:10 GX:0-8 GW:10 BX:0-8 BW:10",
    13: "RW:0-9 GW:0-9 BW:0-9 RX:0-7 RW:11-10 GX:0-7 GW:11-10 BX:0-7 BW:11-10",
    14: "RW:0-9 GW:0-9 BW:0-9 RX:0-3 RW:15-10 GX:0-3 GW:15-10 BX:0-3 BW:15-10",
}
# region of texel t = 4 row + column under partition k, as the format prints them
PARTITIONS = [
    "0011001100110011", "0001000100010001", "0111011101110111", "0001001100110111", "0000000100010011", "0011011101111111", "0001001101111111", "0000000100110111",
    "0000000000010011", "0011011111111111", "0000000101111111", "0000000000010111", "0001011111111111", "0000000011111111", "0000111111111111", "0000000000001111",
    "0000100011101111", "0111000100000000", "0000000010001110", "0111001100010000", "0011000100000000", "0000100011001110", "0000000010001100", "0111001100110001",
    "0011000100010000", "0000100010001100", "0110011001100110", "0011011001101100", "0001011111101000", "0000111111110000", "0111000110001110", "0011100110011100"]
ANCHORS = [15] * 16 + [15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2]      # the anchor texel of region 1; region 0's is texel 0
WEIGHTS = {3: (0, 9, 18, 27, 37, 46, 55, 64), 4: (0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64)}
# what the encoder may emit: quality 1 tries these per partition, highest precision first (mode, precision, delta bits)
TWO_REGION_CHOICES = ((1, 10, 5), (6, 9, 5), (2, 7, 6), (10, 6, 0))

_PART = np.array([[int(c) for c in s] for s in PARTITIONS], np.int64)      # (32, 16)
_ANCHOR = np.array(ANCHORS, np.int64)


def layout_bits(mode):
    """[(field, bit of the field)] for bits 0 ... of the block, the mode bits ("M") included."""
    value, count = MODES[mode][:2]
    out = [("M", k) for k in range(count)]
    for token in LAYOUTS[mode].split():
        name, span = token.split(":")
        a, _, b = span.partition("-")
        a, b = int(a), int(b or a)
        out += [(name, k) for k in (range(a, b + 1) if b >= a else range(a, b - 1, -1))]
    assert len(out) == (82 if MODES[mode][4] == 2 else 65), mode
    return out


def unquantise(x, p):
    """The format's unsigned rule on an integer array of p-bit values."""
    x = np.asarray(x, np.int64)
    if p >= 15:
        return x
    mid = ((x << 16) + 0x8000) >> p
    return np.where(x == 0, 0, np.where(x == (1 << p) - 1, 0xFFFF, mid))


def palette(a, b, index_bits):
    """(..., 3) unquantised ends -> (..., n, 3) decoded half integers: the interpolation, then the final step."""
    w = np.array(WEIGHTS[index_bits], np.int64).reshape((1,) * (a.ndim - 1) + (-1, 1))
    v = (a[..., None, :] * (64 - w) + b[..., None, :] * w + 32) >> 6
    return (v * 31) >> 6


def _split(data, n):
    raw = np.frombuffer(bytes(data), np.uint64, 2 * n)
    return raw[0::2].copy(), raw[1::2].copy()


def _bit(lo, hi, pos):
    return ((lo >> np.uint64(pos)) if pos < 64 else (hi >> np.uint64(pos - 64))).astype(np.int64) & 1


def block_modes(data, n):
    """The mode number 1 ... 14 of each of n blocks; 0 for a reserved value."""
    lo, _ = _split(data, n)
    low5 = (lo & np.uint64(31)).astype(np.int64)
    out = np.zeros(n, np.int64)
    for mode, (value, count, _, _, _) in MODES.items():
        out[(low5 & ((1 << count) - 1)) == value] = mode
    return out


def decode_fields(data, n):
    """n blocks -> (mode (n,), ends (n, 4, 3) as p-bit integers W X Y Z after the transform, partition (n,), indices (n, 16))."""
    lo, hi = _split(data, n)
    modes = block_modes(data, n)
    ends, part, idx = np.zeros((n, 4, 3), np.int64), np.zeros(n, np.int64), np.zeros((n, 16), np.int64)
    for mode in MODES:
        sel = np.nonzero(modes == mode)[0]
        if not len(sel):
            continue
        _, _, p, delta, regions = MODES[mode]
        l, h = lo[sel], hi[sel]
        f = {c + e: np.zeros(len(sel), np.int64) for c in "RGB" for e in "WXYZ"}
        f["D"], f["M"] = np.zeros(len(sel), np.int64), np.zeros(len(sel), np.int64)
        for pos, (name, k) in enumerate(layout_bits(mode)):
            f[name] |= _bit(l, h, pos) << k
        e = np.stack([np.stack([f[c + e_] for c in "RGB"], -1) for e_ in "WXYZ"], 1)      # (m, 4, 3)
        if any(delta):
            for c in range(3):
                d = e[:, 1:, c]
                d = np.where(d >= (1 << (delta[c] - 1)), d - (1 << delta[c]), d)      # sign extension
                e[:, 1:, c] = (e[:, :1, c] + d) & ((1 << p) - 1)                      # and the wrap
        ib = 3 if regions == 2 else 4
        anchor = _ANCHOR[f["D"]] if regions == 2 else np.zeros(len(sel), np.int64)
        pos = np.full(len(sel), (82 if regions == 2 else 65) - 64, np.int64)
        for t in range(16):
            nb = ib - ((t == 0) | ((anchor == t) & (regions == 2))).astype(np.int64)
            idx[sel, t] = (h >> pos.astype(np.uint64)).astype(np.int64) & ((1 << nb) - 1)
            pos += nb
        ends[sel], part[sel] = e, f["D"]
    return modes, ends, part, idx


def decode_texels(data, n):
    """n blocks -> (n, 16, 3) int64 half integers, texel t = 4 row + column."""
    modes, ends, part, idx = decode_fields(data, n)
    out = np.zeros((n, 16, 3), np.int64)
    for mode in MODES:
        sel = np.nonzero(modes == mode)[0]
        if not len(sel):
            continue
        p, regions = MODES[mode][2], MODES[mode][4]
        u = unquantise(ends[sel], p)
        if regions == 1:
            pal = palette(u[:, 0], u[:, 1], 4)[:, None].repeat(16, 1)                                 # (m, 16, n, 3)
        else:
            region = _PART[part[sel]]                                                              # (m, 16)
            both = np.stack([palette(u[:, 0], u[:, 1], 3), palette(u[:, 2], u[:, 3], 3)], 1)      # (m, 2, 8, 3)
            pal = both[np.arange(len(sel))[:, None], region]
        out[sel] = np.take_along_axis(pal, idx[sel][:, :, None, None].repeat(3, 3), 2)[:, :, 0]
    return out


def _blocks_of(w, h):
    return (w + 3) // 4, (h + 3) // 4


def decode_blocks(data, w, h):
    bw, bh = _blocks_of(w, h)
    if len(data) != 16 * bw * bh:
        raise DdsError("%d bytes, a %d x %d image takes %d" % (len(data), w, h, 16 * bw * bh))
    t = decode_texels(data, bw * bh).reshape(bh, bw, 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(4 * bh, 4 * bw, 3)
    return t[:h, :w].astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------- the encoder, the header's steps
def to_half(image):
    """TEXEL TO HALF: float32 -> the EXR output's half, then a set sign bit gives 0.  int64, 0 ... 0x7BFF."""
    bits = half_bits(image).astype(np.int64)
    return np.where(bits & 0x8000, 0, bits)


def blocks_from_image(half):
    """(h, w, 3) -> (blocks, 16, 3) int64, coordinates clamped to the image."""
    half = np.asarray(half, np.int64)
    h, w = half.shape[:2]
    bw, bh = _blocks_of(w, h)
    ys, xs = np.minimum(np.arange(4 * bh), h - 1), np.minimum(np.arange(4 * bw), w - 1)
    full = half[ys][:, xs]
    return full.reshape(bh, 4, bw, 4, 3).transpose(0, 2, 1, 3, 4).reshape(bh * bw, 16, 3)


def quantise(h, p):
    return np.minimum(((h * 64) // 31) >> (16 - p), (1 << p) - 1)


def candidate(px, partition, p, index_bits):
    """Steps 1 - 4 for blocks px (B, 16, 3) under `partition` (None: one region): -> ends (B, 2, 2, 3) quantised [region][end], indices (B, 16),
    error (B,)."""
    B = px.shape[0]
    region, anchor1 = (np.zeros(16, np.int64), None) if partition is None else (_PART[partition], ANCHORS[partition])
    n_idx = 1 << index_bits
    q = np.zeros((B, 2, 2, 3), np.int64)
    idx, err = np.zeros((B, 16), np.int64), np.zeros(B, np.int64)
    for r in range(2 if region.any() else 1):
        t = np.nonzero(region == r)[0]
        v = px[:, t]                                                     # (B, n, 3)
        lo, hi, n = v.min(1), v.max(1), len(t)
        s = v.sum(1)
        for c in (1, 2):                                                 # the diagonal: G against R, B against R
            cov = n * (v[..., 0] * v[..., c]).sum(1) - s[:, 0] * s[:, c]
            swap = cov < 0
            lo[:, c], hi[:, c] = np.where(swap, hi[:, c], lo[:, c]), np.where(swap, lo[:, c], hi[:, c])
        qa, qb = quantise(lo, p), quantise(hi, p)
        pal = palette(unquantise(qa, p), unquantise(qb, p), index_bits)      # (B, n_idx, 3)
        d = ((pal[:, None] - v[:, :, None]) ** 2).sum(-1)                # (B, n, n_idx)
        best = d.argmin(-1)                                              # the first least: ties to the lower index
        err += d.min(-1).sum(1)
        flip = best[:, list(t).index(0 if r == 0 else anchor1)] >= n_idx // 2      # the anchor's top bit
        best = np.where(flip[:, None], n_idx - 1 - best, best)
        q[:, r, 0], q[:, r, 1] = np.where(flip[:, None], qb, qa), np.where(flip[:, None], qa, qb)
        idx[:, t] = best
    return q, idx, err


def feasible(q, delta_bits):
    """Step 5: every delta against region 0's first end fits its signed field."""
    if not delta_bits:
        return np.ones(q.shape[0], bool)
    d = q.reshape(q.shape[0], 4, 3)[:, 1:] - q[:, 0, 0][:, None]
    return ((d >= -(1 << (delta_bits - 1))) & (d < (1 << (delta_bits - 1)))).all((1, 2))


def pack(mode, q, part, idx):
    """Blocks of one mode -> (B, 2) uint64.  q (B, 2, 2, 3) are the ends themselves; the deltas of a transformed mode are made here."""
    value, count, p, delta, regions = MODES[mode]
    B = q.shape[0]
    e = q.reshape(B, 4, 3).copy()
    if any(delta):
        for c in range(3):
            e[:, 1:, c] = (e[:, 1:, c] - e[:, :1, c]) & ((1 << delta[c]) - 1)
    f = {c + n: e[:, k, j] for j, c in enumerate("RGB") for k, n in enumerate("WXYZ")}
    f["D"], f["M"] = np.asarray(part, np.int64) + np.zeros(B, np.int64), np.full(B, value, np.int64)
    words = np.zeros((B, 2), np.uint64)
    for pos, (name, k) in enumerate(layout_bits(mode)):
        words[:, pos // 64] |= (((f[name] >> k) & 1).astype(np.uint64)) << np.uint64(pos % 64)
    ib = 3 if regions == 2 else 4
    anchor = _ANCHOR[f["D"]] if regions == 2 else np.zeros(B, np.int64)
    pos = np.full(B, (82 if regions == 2 else 65) - 64, np.int64)
    for t in range(16):
        nb = ib - ((t == 0) | ((anchor == t) & (regions == 2))).astype(np.int64)
        assert (idx[:, t] < (1 << nb)).all(), "an anchor index with its top bit set"
        words[:, 1] |= idx[:, t].astype(np.uint64) << pos.astype(np.uint64)
        pos += nb
    return words


def encode_texels(px, quality, chunk=4096, detail=False):
    """(B, 16, 3) half integers -> (B, 2) uint64 blocks [, mode, partition, error] by the header's candidates and choice."""
    if quality not in (0, 1):
        raise ValueError("quality must be 0 or 1")
    px = np.asarray(px, np.int64)
    B = px.shape[0]
    words, modes, parts, errs = np.zeros((B, 2), np.uint64), np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    for at in range(0, B, chunk):
        v = px[at:at + chunk]
        q, idx, err = candidate(v, None, 10, 4)
        w, m, pt = pack(11, q, 0, idx), np.full(len(v), 11, np.int64), np.zeros(len(v), np.int64)
        for k in range(32 if quality else 0):
            open_ = np.ones(len(v), bool)                      # no mode taken yet for partition k
            for mode, p, d in TWO_REGION_CHOICES:
                q2, idx2, err2 = candidate(v, k, p, 3)
                take = open_ & feasible(q2, d)
                open_ &= ~take
                better = take & (err2 < err)                   # strictly: ties stay with mode 11, then the lower partition
                if better.any():
                    w[better] = pack(mode, q2[better], k, idx2[better])
                    m[better], pt[better], err[better] = mode, k, err2[better]
        words[at:at + chunk], modes[at:at + chunk], parts[at:at + chunk], errs[at:at + chunk] = w, m, pt, err
    return (words, modes, parts, errs) if detail else words


def encode_blocks(half, quality=0):
    return encode_texels(blocks_from_image(half), quality).tobytes()


# ---------------------------------------------------------------------------------------------------------------- the file
def level_blocks(e):
    return max(1, e // 4) ** 2


def header(edge, levels):
    w = [0] * 37
    w[0], w[1], w[2] = 0x20534444, 124, 0x000A1007      # CAPS | HEIGHT | WIDTH | PIXELFORMAT | MIPMAPCOUNT | LINEARSIZE
    w[3], w[4], w[5], w[7] = edge, edge, 16 * level_blocks(edge), levels
    w[19], w[20], w[21] = 32, 0x4, 0x30315844
    w[27], w[28] = 0x00401008, 0x0000FE00
    w[32], w[33], w[34], w[35] = DXGI_BC6H_UF16, 3, 0x4, 1
    return struct.pack("<37I", *w)


def file_bytes(edge, levels):
    return HEADER_BYTES + 6 * 16 * sum(level_blocks(edge >> l) for l in range(levels))


def write(levels, quality=0):
    levels = [to_half(v) if np.asarray(v).dtype.kind == "f" else np.asarray(v, np.int64) for v in levels]
    E = levels[0].shape[1]
    for l, v in enumerate(levels):
        if (E >> l) < 1 or v.shape != (6, E >> l, E >> l, 3):
            raise DdsError("level %d must have shape (6, %d, %d, 3)" % (l, E >> l, E >> l))
        if v.min() < 0 or v.max() > HALF_MAX:
            raise DdsError("half integers must lie in 0 ... 0x7BFF")
    parts = [header(E, len(levels))]
    for face in range(6):
        for v in levels:
            parts.append(encode_blocks(v[face], quality))
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
    if w[32] != DXGI_BC6H_UF16:
        raise DdsError("DXGI format %d: only BC6H_UF16 (95) is read" % w[32])
    if w[33] != 3 or not (w[34] & 0x4) or w[35] != 1 or (w[28] & 0xFE00) != 0xFE00:
        raise DdsError("not a single complete cube map (dimension, TEXTURECUBE, array size, caps2)")
    E, L = w[4], w[7]
    if w[3] != E or E < 1 or (E & (E - 1)):
        raise DdsError("height and width must be the same power of two")
    if L < 1 or (E >> (L - 1)) < 1:
        raise DdsError("mipMapCount %d does not fit edge %d" % (L, E))
    if not (w[2] & 0x00080000) or (w[2] & 0x8) or w[5] != 16 * level_blocks(E):
        raise DdsError("LINEARSIZE must be set, PITCH clear, and the linear size that of level 0 of one face")
    if len(data) != file_bytes(E, L):
        raise DdsError("%d bytes, the header asks for %d" % (len(data), file_bytes(E, L)))
    levels = [np.empty((6, E >> l, E >> l, 3), np.uint16) for l in range(L)]
    at = HEADER_BYTES
    for face in range(6):
        for l in range(L):
            e = E >> l
            n = 16 * level_blocks(e)
            levels[l][face] = decode_blocks(data[at:at + n], e, e)
            at += n
    return levels, dict(edge=E, levels=L)
