"""What a 1D and a 3D lookup table MEAN, in float64, written as loops from the definitions: the yardstick tests/test_look_ref.py holds the float32
restatement (tests/look_ref.py) to.  It shares no code with that file and does not follow the header's order of operations.

A 1D table is the piecewise-linear function through its entries.  A 3D table, trilinear: the tensor product of that, the weighted sum over the
cell's eight corners.  Tetrahedral: the piecewise-linear interpolant over the Kuhn triangulation of the cell — walk from corner (0, 0, 0) to
corner (1, 1, 1) one axis at a time, the axes in the order of their fractions, largest first; the point is the corner reached so far plus what is
left of each step, and the interpolant adds, per step, that fraction of the difference along the step."""
import math

import numpy as np


def _axis(x, lo, hi, n):
    """Cell and fraction of x on an axis of n entries spanning [lo, hi]; outside the span the ends hold."""
    t = (float(x) - lo) * (n - 1) / (hi - lo)
    t = min(max(t, 0.0), float(n - 1))
    cell = min(int(math.floor(t)), n - 2)
    return cell, t - cell


def curve(x, T, lo, hi):
    n = len(T)
    cell, f = _axis(x, lo, hi, n)
    return T[cell] + f * (T[cell + 1] - T[cell])


def trilinear(p, T, lo, hi):
    n = T.shape[0]
    (ir, fr), (ig, fg), (ib, fb) = (_axis(p[c], lo[c], hi[c], n) for c in range(3))
    y = np.zeros(3)
    for B in (0, 1):
        for G in (0, 1):
            for R in (0, 1):
                w = (fr if R else 1.0 - fr) * (fg if G else 1.0 - fg) * (fb if B else 1.0 - fb)
                y += w * T[ib + B, ig + G, ir + R]
    return y


def tetrahedral(p, T, lo, hi):
    n = T.shape[0]
    cells, fracs = zip(*(_axis(p[c], lo[c], hi[c], n) for c in range(3)))
    at = [cells[2], cells[1], cells[0]]              # index into T[b][g][r]
    y = T[tuple(at)].copy()
    for axis in sorted(range(3), key=lambda c: -fracs[c]):
        here = T[tuple(at)]
        at[2 - axis] += 1
        y += fracs[axis] * (T[tuple(at)] - here)
    return y


def apply(x, cube=None, shaper=None, strength=1.0, interpolation="tetrahedral"):
    """(n, 3) finite pixels through the tables (digital_earth_amd.cube.Cube), the mix and the clamp; float64 out."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    T1 = np.array(shaper.table, dtype=np.float64).reshape(shaper.size, 3) if shaper is not None else None
    T3 = np.array(cube.table, dtype=np.float64).reshape(cube.size, cube.size, cube.size, 3) if cube is not None else None
    lo1 = hi1 = lo3 = hi3 = None
    if shaper is not None:
        lo1, hi1 = [float(np.float32(v)) for v in shaper.domain_min], [float(np.float32(v)) for v in shaper.domain_max]
    if cube is not None:
        lo3, hi3 = [float(np.float32(v)) for v in cube.domain_min], [float(np.float32(v)) for v in cube.domain_max]
    solid = tetrahedral if interpolation == "tetrahedral" else trilinear
    s = float(np.float32(strength))
    out = np.empty_like(x)
    for k in range(x.shape[0]):
        y = x[k]
        if T1 is not None:
            y = np.array([curve(y[c], T1[:, c], lo1[c], hi1[c]) for c in range(3)])
        if T3 is not None:
            y = solid(y, T3, lo3, hi3)
        out[k] = np.clip(x[k] * (1.0 - s) + y * s, 0.0, 1.0)
    return out
