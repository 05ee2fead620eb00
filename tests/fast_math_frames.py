"""The paired-sample statistic of tests/test_gpu_fast_math_frames.py, on the CPU: stacks C[s], F[s] of single-sample frames (flag off / on, the same seed,
pixels and sample indices) -> per region z = mean(D) / (std(D) / sqrt(n)) on the luminance of D = F - C.  Only the samples that took another path differ,
so D carries a fraction of either frame's variance and a bias of a few 1e-3 in one region shows where a whole-frame 1 % check cannot see it."""
import numpy as np

LUMA = np.array([0.2126, 0.7152, 0.0722])
BLOCKS = (4, 2)          # the fixed partition: 4 x 2 = 8 blocks of the frame
MIN_MOVED = 500          # a region with fewer moved samples is merged with its neighbour: the normal approximation needs them
Z_MAX = 5.0


def luminance(stack):
    return np.asarray(stack, np.float64) @ LUMA


def moved_mask(C, F):
    """Samples on another path, as tests/test_gpu_round5.py counts them: the sum of the channels moves by more than 1e-3 relative."""
    c, f = np.asarray(C, np.float64).sum(-1), np.asarray(F, np.float64).sum(-1)
    return np.abs(f - c) > 1e-3 * np.maximum(np.abs(c), np.abs(f))


def regions(moved):
    """Boolean masks (W, H) of the regions: the blocks of the fixed partition in raster order, a block with fewer than MIN_MOVED moved samples joined to the
    next one (the last group to the one before it)."""
    N, W, H = moved.shape
    bx, by = BLOCKS
    blocks = []
    for j in range(by):
        for i in range(bx):
            m = np.zeros((W, H), bool)
            m[i * W // bx:(i + 1) * W // bx, j * H // by:(j + 1) * H // by] = True
            blocks.append(m)
    groups, cur = [], None
    for m in blocks:
        cur = m if cur is None else (cur | m)
        if moved[:, cur].sum() >= MIN_MOVED:
            groups.append(cur); cur = None
    if cur is not None:
        if groups: groups[-1] = groups[-1] | cur
        else: groups.append(cur)
    return groups


def z_value(D):
    """mean(D) / (std(D) / sqrt(n)) over all the pixel-samples of D; 0 where nothing differs."""
    D = np.asarray(D, np.float64).ravel()
    s = D.std()
    return 0.0 if s == 0.0 else float(D.mean() / (s / np.sqrt(D.size)))


def paired_z(C, F):
    """[(name, pixel-samples, moved samples, z)] for the whole frame and every region."""
    moved = moved_mask(C, F)
    D = luminance(F) - luminance(C)
    out = [("frame", D.size, int(moved.sum()), z_value(D))]
    for k, m in enumerate(regions(moved)):
        out.append(("region %d" % k, int(D[:, m].size), int(moved[:, m].sum()), z_value(D[:, m])))
    return out


DELTAS = tuple(10.0 ** e for e in np.arange(-4.0, -0.99, 0.125))


def detectable_delta(C, F, mask=None):
    """The smallest delta of DELTAS from which on F scaled by (1 + delta) AND by (1 - delta) is rejected (|z| > Z_MAX) at every larger delta too."""
    yc, yf = luminance(C), luminance(F)
    if mask is not None:
        yc, yf = yc[:, mask], yf[:, mask]
    best = None
    for d in reversed(DELTAS):
        if all(abs(z_value(yf * (1.0 + s * d) - yc)) > Z_MAX for s in (1.0, -1.0)):
            best = d
        else:
            break
    return best


def proportional(C, F, tol=1e-5):
    """The wavelength of a sample is drawn before anything the flag touches and fixes the colour of its radiance: wherever both frames are lit, rgb_F and rgb_C
    are proportional — |F_i C_j - F_j C_i| <= tol |F| |C| (tol: a dozen float32 roundings, the two sides taking different ones).  Returns the worst ratio."""
    C, F = np.asarray(C, np.float64), np.asarray(F, np.float64)
    lit = (np.abs(C).max(-1) > 0) & (np.abs(F).max(-1) > 0)
    c, f = C[lit], F[lit]
    cross = np.stack([f[:, 0] * c[:, 1] - f[:, 1] * c[:, 0], f[:, 1] * c[:, 2] - f[:, 2] * c[:, 1], f[:, 2] * c[:, 0] - f[:, 0] * c[:, 2]], -1)
    scale = np.linalg.norm(c, axis=1) * np.linalg.norm(f, axis=1)
    return float((np.abs(cross).max(-1) / scale).max()) if lit.any() else 0.0, int(lit.sum())
