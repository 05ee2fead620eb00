"""The Radiance HDR output restated in numpy (include/digital_earth_rgbe.h): the sample in integers on the float32 bits, the run-length policy, the
front, the capacity.  The GPU's file equals encode() byte for byte (tests/test_gpu_rgbe.py); nothing here is shared with the library or with
digital_earth_amd/rgbe.py."""
import numpy as np

F = np.float32
ROUNDINGS = {"trunc": 0, "round": 1}
CLAMP_BITS = 0x7EFF0000                                            # 255 2^119
TINY_BITS = int(np.float32(1e-32).view(np.uint32))
MAX_FLAT = 1 << 27
PRIMARIES = "0.64 0.33 0.3 0.6 0.15 0.06 0.3127 0.329"


def pixels(image, scale=1.0, rounding="trunc"):
    """(..., 3) float32 -> (..., 4) uint8 R, G, B, E: steps 1 to 7 of the header, in int64 on the bits."""
    v = np.asarray(image, F) * F(scale)                            # one float32 multiplication
    x = np.ascontiguousarray(v).view(np.uint32).astype(np.int64)
    x = np.where((x >> 31 != 0) | (x > 0x7F800000), 0, np.minimum(x, CLAMP_BITS))      # NaN and negative -> +0; the clamp
    m = x.max(axis=-1)
    em = (m >> 23)[..., None]
    ec = x >> 23
    M = np.where(ec == 0, 0, (x & 0x7FFFFF) | 0x800000)

    def quantise(carry):
        sh = np.minimum(16 + em - ec + carry, 40)                  # M < 2^24: every shift from 25 on gives 0
        return (M + (1 << (sh - 1))) >> sh if rounding == "round" else M >> sh
    q = quantise(0)
    up = (q == 256).any(axis=-1)
    q = np.where(up[..., None], quantise(1), q)
    E = em[..., 0] + 2 + up
    assert (E <= 255).all() and (q <= 255).all()                   # the clamp keeps every pixel below the format's end
    out = np.concatenate([q, E[..., None]], axis=-1).astype(np.uint8)
    out[m < TINY_BITS] = 0
    return out


def encode_plane(p):
    """One plane's bytes: stretches of >= 4 equal bytes as runs of at most 127, the rest as literal packets of at most 128."""
    p = np.asarray(p, np.uint8)
    W = len(p)
    starts = np.concatenate([[0], np.flatnonzero(p[1:] != p[:-1]) + 1, [W]])
    out, lit = bytearray(), []

    def flush():
        if lit:
            data = np.concatenate(lit).tobytes()
            for k in range(0, len(data), 128):
                out.append(min(128, len(data) - k))
                out.extend(data[k:k + 128])
            del lit[:]
    for a, b in zip(starts[:-1], starts[1:]):
        L = int(b - a)
        if L >= 4:
            flush()
            out.extend(bytes((0xFF, int(p[a]))) * (L // 127))
            if L % 127:
                out.extend(bytes((0x80 + L % 127, int(p[a]))))
        else:
            lit.append(p[a:b])
    flush()
    return bytes(out)


def is_rle(W, rle=True):
    return bool(rle) and 8 <= W <= 32767


def front(W, H, scale=1.0):
    text = "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\nPRIMARIES=%s\n" % PRIMARIES
    if F(scale) != F(1.0):
        text += "EXPOSURE=%.9g\n" % float(F(scale))
    return (text + "\n-Y %d +X %d\n" % (H, W)).encode()


def plane_bound(W):
    return W + (W + 127) // 128


def capacity(W, H, rle=True, scale=1.0):
    return len(front(W, H, scale)) + H * (4 + 4 * plane_bound(W) if is_rle(W, rle) else 4 * W)


def encode(image, rle=True, rounding="trunc", scale=1.0):
    image = np.asarray(image, F)
    H, W = image.shape[:2]
    px = pixels(image, scale, rounding)
    parts = [front(W, H, scale)]
    if not is_rle(W, rle):
        return parts[0] + px.tobytes()
    for y in range(H):
        parts.append(bytes((2, 2, W >> 8, W & 255)))
        for c in range(4):
            parts.append(encode_plane(px[y, :, c]))
    return b"".join(parts)
