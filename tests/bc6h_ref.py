"""The BC6H encoder of include/digital_earth_ibl_bc6h.h over whole images, in numpy, vectorised over blocks (no per-block Python loop): the steps
themselves are stated once, in digital_earth_amd/bc6h.py (candidate, feasible, pack, encode_texels), because bc6h.write needs them inside the package;
this module carries what the tests add: float images in, the header's error metric, an exhaustive index search, hand-assembly of blocks."""
import numpy as np

from digital_earth_amd import bc6h

FIELDS = ["struct_bytes", "on", "quality"]
STRUCT_BYTES = 12
EMITTED = {11, 1, 6, 2, 10}


def encode(image, quality):
    """(h, w, 3) float32 -> the blocks' bytes."""
    return bc6h.encode_blocks(bc6h.to_half(image), quality)


def encode_detail(image, quality):
    """-> (bytes, mode (B,), partition (B,), claimed error (B,), the blocks' texels (B, 16, 3))."""
    px = bc6h.blocks_from_image(bc6h.to_half(image))
    words, modes, parts, errs = bc6h.encode_texels(px, quality, detail=True)
    return words.tobytes(), modes, parts, errs, px


def block_error(data, px):
    """The header's metric per block: sum over texels and channels of (decoded - texel)^2."""
    return ((bc6h.decode_texels(data, px.shape[0]) - px) ** 2).sum((1, 2))


def least_index_error(data, px):
    """For the ends each block carries, the least error any choice of indices reaches: per texel the minimum over the texel's region's palette."""
    n = px.shape[0]
    modes, ends, part, _ = bc6h.decode_fields(data, n)
    out = np.zeros(n, np.int64)
    for b in range(n):
        _, _, p, _, regions = bc6h.MODES[int(modes[b])]
        u = bc6h.unquantise(ends[b], p)
        for t in range(16):
            r = int(bc6h.PARTITIONS[int(part[b])][t]) if regions == 2 else 0
            pal = bc6h.palette(u[2 * r], u[2 * r + 1], 3 if regions == 2 else 4)
            out[b] += ((pal - px[b, t]) ** 2).sum(-1).min()
    return out


def assemble(mode, fields, indices):
    """One block by hand: fields {"RW": ..., "D": ...} as the raw field values (deltas as two's complement of their width), indices 16 integers."""
    value, count, _, _, regions = bc6h.MODES[mode]
    block, f = 0, dict(fields, M=value)
    for pos, (name, k) in enumerate(bc6h.layout_bits(mode)):
        block |= ((f.get(name, 0) >> k) & 1) << pos
    pos, ib = (82, 3) if regions == 2 else (65, 4)
    anchor = bc6h.ANCHORS[f.get("D", 0)] if regions == 2 else 0
    for t in range(16):
        nb = ib - (1 if t == 0 or (regions == 2 and t == anchor) else 0)
        assert 0 <= indices[t] < (1 << nb)
        block |= indices[t] << pos
        pos += nb
    assert pos == 128
    return block.to_bytes(16, "little")


def test_image(w, h, seed=0):
    """A seeded smooth field with a hard edge and a 3-texel sun of 7e4, with zeros, negatives, NaN and +-Inf."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([0.2 + 0.011 * xx + 0.02 * yy, 0.5 + 0.3 * np.sin(0.21 * xx + 0.1 * yy), 0.1 + 0.003 * yy * xx], -1) * (1 + 0.05 * rng.random((h, w, 3)))
    img[:, w // 2:] *= 6.0
    img[:, w // 2:, 1] = 0.02
    img = img.astype(np.float32)
    if w >= 8 and h >= 7:
        img[3, 2:5] = 7e4
        img[5, 1] = [np.nan, -1.0, np.inf]
        img[6, 6] = [-np.inf, 0.0, 0.0]
        img[0:4, 0:2] = 0.0
    return img
