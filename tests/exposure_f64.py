"""A numpy restatement of the auto-exposure meter (include/digital_earth_exposure.h): the bin function, the bins' centres, the trimmed
mean and the EV update.  It shares no code with csrc/: the bin function is f32 operations in the stated order with the bins read from the bit
pattern (view(np.uint32)), everything after the integer histogram is float64."""
import numpy as np

BINS = 256
Y_MIN = np.float32(2.0 ** -24)
Y_MAX = np.float32(2.0 ** 8)
DEFAULTS = dict(key=0.18, compensation=0.0, ev_range=(-8.0, 16.0), percentiles=(0.10, 0.95), adapt=1.0, region=None)


def luminance(mean_rgb):
    """Y = (0.2126 r + 0.7152 g) + 0.0722 b in f32, no contraction.  mean_rgb: (..., 3) float32."""
    m = np.asarray(mean_rgb, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (np.float32(0.2126) * m[..., 0] + np.float32(0.7152) * m[..., 1]) + np.float32(0.0722) * m[..., 2]


def bin_of(Y):
    """(bin, below, clipped) of f32 luminances: bin = min((bits >> 20) - 824, 255) where Y >= 2^-24 (else `below`: zero, negatives, NaN; bin -1);
    clipped where Y >= 2^8 (those sit in bin 255)."""
    Y = np.asarray(Y, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        metered = Y >= Y_MIN
        clipped = Y >= Y_MAX
    u = np.ascontiguousarray(Y).view(np.uint32).astype(np.int64)
    b = np.minimum((u >> 20) - 824, 255)
    return np.where(metered, b, -1), ~metered, clipped


def centres():
    """log2 of the centre of every bin: bin k is sub-bin k & 7 (of 8 linear ones) of octave (k >> 3) - 24."""
    k = np.arange(BINS)
    return (k >> 3).astype(np.float64) - 24.0 + np.log2(1.0 + ((k & 7).astype(np.float64) + 0.5) / 8.0)


def bin_edges():
    """The 257 edges of the bins as exact float64 luminances."""
    k = np.arange(BINS + 1)
    return np.ldexp(1.0 + (k & 7) / 8.0, (k >> 3) - 24)


def meter(sums, samples, region=None):
    """The histogram of what the display reads.  sums: (W, H, 3) float32 in fetch_hdr's layout; samples: a scalar count, or a (W, H) array of per-pixel
    counts (an adaptive frame's tile counts, expanded).  The division is the display's own: f32 sum / f32 count.  region = (x0, y0, x1, y1), half-open."""
    s = np.asarray(sums, dtype=np.float32)
    n = np.asarray(samples).astype(np.float32)
    if n.ndim == 2:
        n = n[..., None]
    with np.errstate(all="ignore"):
        mean = s / n
    Y = luminance(mean)
    if region is not None:
        x0, y0, x1, y1 = region
        Y = Y[x0:x1, y0:y1]
    b, below, clipped = bin_of(Y.ravel())
    hist = np.bincount(b[b >= 0], minlength=BINS).astype(np.uint32)
    return dict(histogram=hist, metered=int(hist.sum(dtype=np.uint64)), below=int(below.sum()), clipped=int(clipped.sum()))


def trimmed_mean(hist, low_fraction, high_fraction):
    """The mean of the bins' centres over the pixels of rank [lo, hi) in ascending luminance: lo = floor(low N), hi = floor(high N) with the f32
    fractions widened to double, hi = lo + 1 when they coincide.  None when the histogram is empty."""
    h = [int(x) for x in hist]
    N = sum(h)
    if N == 0:
        return None
    lo = int(np.floor(np.float64(np.float32(low_fraction)) * np.float64(N)))
    hi = int(np.floor(np.float64(np.float32(high_fraction)) * np.float64(N)))
    if hi == lo:
        hi = lo + 1
    c = centres()
    acc, kept, C = np.float64(0.0), 0, 0
    for k in range(BINS):
        r = max(0, min(C + h[k], hi) - max(C, lo))
        if r > 0:
            acc = acc + np.float64(r) * c[k]
            kept += r
        C += h[k]
    return acc / np.float64(kept)


class Meter:
    """The EV recurrence of one context: update(hist, manual) per display; clear() is what de_set_auto_exposure does."""

    def __init__(self, key=0.18, compensation=0.0, ev_range=(-8.0, 16.0), percentiles=(0.10, 0.95), adapt=1.0, region=None):
        self.key, self.compensation, self.ev_range, self.percentiles, self.adapt, self.region = key, compensation, ev_range, percentiles, adapt, region
        self.prev = None

    def clear(self):
        self.prev = None

    def update(self, hist, manual_exposure=0.0):
        """Returns dict(ev, ev_target, mean_log2, valid): ev as the f32 the display uses, the other two in float64."""
        mean = trimmed_mean(hist, *self.percentiles)
        if mean is None:      # all black: the exposure stays (the manual one while there is no previous EV), and no state is made
            ev = np.float32(self.prev if self.prev is not None else np.float32(manual_exposure))
            return dict(ev=float(ev), ev_target=float(ev), mean_log2=0.0, valid=False)
        f = lambda x: np.float64(np.float32(x))
        target = (np.log2(f(self.key)) - mean) + f(self.compensation)
        target = min(max(target, f(self.ev_range[0])), f(self.ev_range[1]))
        ev = target if self.prev is None else self.prev + f(self.adapt) * (target - self.prev)
        ev32 = np.float32(ev)
        self.prev = np.float64(ev32)
        return dict(ev=float(ev32), ev_target=float(target), mean_log2=float(mean), valid=True)


def ulps_f32(a, b):
    """Distance of two values in units of the f32 spacing at the larger magnitude (both are first rounded to f32)."""
    a32, b32 = np.float32(a), np.float32(b)
    if a32 == b32:
        return 0.0
    return float(abs(np.float64(a32) - np.float64(b32)) / np.float64(np.spacing(np.float32(max(abs(a32), abs(b32))))))
