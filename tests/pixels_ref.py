"""The 8-bit pixel output (include/digital_earth_pixels.h) restated in numpy: uint32 and float32 only on the value path, every operation
in the order the header states, so that the device's bytes can be held to it exactly.

    pack(image, channels, mode, seed, phase)  ->  (H, W, channels) uint8, row 0 at the top

image is the display's output: (W, H, 3) float32, image[u, v] with v = 0 at the bottom."""
import numpy as np

MODES = ("truncate", "round", "dither")
DEFAULTS = dict(channels=4, mode="truncate", seed=0, animate=False)
F = np.float32
U = np.uint32


def mix(x):
    """The 32-bit hash (wrapping uint32 arithmetic)."""
    x = np.asarray(x, dtype=U).copy()
    x ^= x >> U(16)
    x *= U(0x7feb352d)
    x ^= x >> U(15)
    x *= U(0x846ca68b)
    x ^= x >> U(16)
    return x


def key(seed, phase):
    """k = mix(seed + 0x9E3779B9 phase); phase may be an array."""
    phase = np.asarray(phase, dtype=np.uint64) & np.uint64(0xffffffff)
    return mix(((np.uint64(int(seed) & 0xffffffff) + np.uint64(0x9E3779B9) * phase) & np.uint64(0xffffffff)).astype(U))      # the sum modulo 2^32


def tri(seed, phase, idx):
    """The triangular noise on (-1, 1) of the hash of (seed, phase, idx): exact in f32."""
    h = mix(key(seed, phase) ^ np.asarray(idx, dtype=U))
    return (h >> U(16)).astype(F) * F(2.0 ** -16) - (h & U(0xffff)).astype(F) * F(2.0 ** -16)


def scaled(t):
    """Steps 1 and 2: s = clamp(t) * 255, with NaN and -0.0 to 0 and +inf to 1."""
    t = np.asarray(t, dtype=F)
    with np.errstate(invalid="ignore"):
        cl = np.where(t > F(0), np.where(t < F(1), t, F(1)), F(0)).astype(F)
    return cl * F(255.0)


def quantise(t, mode, seed=0, phase=0, idx=None):
    """Step 3 on values t; idx (same shape, uint32) = (r W + x) 4 + c is needed by the dither only.  Returns int64 levels (0 ... 255 by the model)."""
    s = scaled(t)
    if mode == "truncate":
        return s.astype(np.int32).astype(np.int64)
    if mode == "round":
        return (s + F(0.5)).astype(np.int32).astype(np.int64)
    if mode != "dither":
        raise ValueError(mode)
    e = F(255.0) - s
    m = np.where(s < e, s, e).astype(F)
    a = np.where(m < F(1), m, F(1)).astype(F)
    return ((s + F(0.5)) + a * tri(seed, phase, idx)).astype(F).astype(np.int32).astype(np.int64)


def indices(W, H):
    """idx[u, v, c] = (r W + x) 4 + c with r = H - 1 - v, x = u, as uint32."""
    u = np.arange(W, dtype=np.int64)[:, None, None]
    v = np.arange(H, dtype=np.int64)[None, :, None]
    c = np.arange(3, dtype=np.int64)[None, None, :]
    return ((((H - 1 - v) * W + u) * 4 + c) & 0xffffffff).astype(U)


def pack(image, channels=4, mode="truncate", seed=0, phase=0):
    image = np.asarray(image, dtype=F)
    W, H = image.shape[:2]
    assert image.shape == (W, H, 3) and channels in (3, 4)
    q = quantise(image, mode, seed, phase, indices(W, H) if mode == "dither" else None)
    assert q.min() >= 0 and q.max() <= 255
    out = np.full((H, W, channels), 255, np.uint8)
    out[..., :3] = q.astype(np.uint8).transpose(1, 0, 2)[::-1]      # out[r][x] = image[x][H - 1 - r]
    return out
