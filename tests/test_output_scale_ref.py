"""The numpy restatement of the output scaling (tests/output_scale_ref.py) against an independent float64 statement of the header's continuous
definition (include/digital_earth_output_scale.h), and its exact properties.  No GPU.

The float64 statement below shares no code with output_scale_ref.weights: it finds the taps of an output sample by testing x - a s < i < x + a s on every
integer of a generous range, evaluates the kernels from their textbook forms (the general Mitchell-Netravali polynomials at B = C = 1/3, numpy's
sinc, max(0, 1 - |t|)), normalises in float64 and applies the dense (n_dst, n_src) matrix with the edge taps accumulated on the edge samples.

With u = 2^-24 (float32's unit roundoff) a pass computes, per value, `taps` products and adds of float32 weights: by the usual bound for a
recursive sum its error against the exact weights is at most (taps + 2) u sum|w| max|v| — one u for the rounding of the weight, one for the product,
and the adds (the first adds to 0.0 and is exact, which leaves room for the correction's residual on the last tap: that residual IS the rounding of
the same weights and the same adds on an image of ones).  The second pass multiplies the error of the first by its own sum|w| and adds its own."""
import numpy as np
import pytest

import output_scale_ref as ref

F = np.float32
U = 2.0 ** -24
PAIRS = [((48, 40), (32, 24)), ((16, 8), (64, 32)), ((64, 64), (16, 8)), ((80, 56), (48, 40)), ((48, 40), (48, 24)), ((208, 120), (112, 72))]
AXES = sorted({(s[k], d[k]) for s, d in PAIRS for k in (0, 1) if s[k] != d[k]} | {(64, 8), (8, 64), (2160, 1080), (544, 1080), (24, 16)})
SUPPORT = {"box": 0.5, "triangle": 1.0, "mitchell": 2.0, "lanczos3": 3.0}


def k64(filter, t):
    t = np.abs(np.asarray(t, np.float64))
    if filter == "box":
        return np.ones_like(t)
    if filter == "triangle":
        return np.maximum(0.0, 1.0 - t)
    if filter == "mitchell":
        B = C = 1.0 / 3.0
        near = ((12 - 9 * B - 6 * C) * t ** 3 + (-18 + 12 * B + 6 * C) * t ** 2 + (6 - 2 * B)) / 6
        far = ((-B - 6 * C) * t ** 3 + (6 * B + 30 * C) * t ** 2 + (-12 * B - 48 * C) * t + (8 * B + 24 * C)) / 6
        return np.where(t < 1, near, np.where(t < 2, far, 0.0))
    return np.where(t < 3, np.sinc(t) * np.sinc(t / 3.0), 0.0)


def taps64(n_src, n_dst, filter):
    """Per output sample: (indices, float64 weights normalised to 1), from the continuous definition."""
    r = n_src / n_dst
    s = max(r, 1.0)
    a = SUPPORT[filter]
    rows = []
    for j in range(n_dst):
        x = (j + 0.5) * r - 0.5
        i = np.arange(int(np.floor(x)) - 60, int(np.floor(x)) + 61)
        i = i[(i > x - a * s) & (i < x + a * s)]      # |i - x| < a s as the header spells it: strictly between x - a s and x + a s
        if len(i) == 0:
            i = np.array([int(np.floor(x + 0.5))])
        w = k64(filter, (i - x) / s)
        rows.append((i, w / w.sum()))
    return rows


def matrix64(n_src, n_dst, filter):
    M = np.zeros((n_dst, n_src))
    for j, (i, w) in enumerate(taps64(n_src, n_dst, filter)):
        np.add.at(M[j], np.clip(i, 0, n_src - 1), w)
    return M


def resample64(image, size, filter):
    W, H = image.shape[:2]
    ow, oh = size
    out = image.astype(np.float64)
    if oh != H:
        out = np.einsum("jv,uvc->ujc", matrix64(H, oh, filter), out)
    if ow != W:
        out = np.einsum("ju,uvc->jvc", matrix64(W, ow, filter), out)
    return np.clip(out, 0.0, 1.0) if (ow, oh) != (W, H) else out


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _image(W, H, seed=0):
    return np.random.default_rng(W * 131 + H + seed).random((W, H, 3), dtype=F)


@pytest.mark.parametrize("filter", ref.FILTERS)
def test_every_row_sums_to_exactly_one_in_float32(filter):
    for n_src, n_dst in AXES:
        first, w = ref.weights(n_src, n_dst, filter)
        assert w.dtype == F and first.dtype == np.int32 and w.shape[1] <= ref.MAX_TAPS
        assert (_bits(ref.row_sums(w)) == _bits(F(1.0))).all(), (n_src, n_dst)
        assert (np.diff(first) >= 0).all() and first[0] <= 0 and first[-1] + w.shape[1] - 1 >= n_src - 1      # ascending; both edges reached
    assert ref.weights(64, 8, "lanczos3")[1].shape[1] <= 49 and ref.weights(2160, 1080, "lanczos3")[1].shape[1] in (12, 13)


@pytest.mark.parametrize("filter", ref.FILTERS)
def test_tables_agree_with_the_float64_weights(filter):
    """Every tap but a row's last is the float64 weight rounded once: within one float32 ulp of the row's largest weight.  The last tap is
    fl(1 - P): it carries, besides, the correction's residual — the roundings of the n - 1 weights before it (each at most u times the largest) and
    of the n - 2 inexact adds of P (each at most u times the partial sum, itself at most sum|w|)."""
    for n_src, n_dst in AXES:
        first, w = ref.weights(n_src, n_dst, filter)
        for j, (i, w64) in enumerate(taps64(n_src, n_dst, filter)):
            n = len(i)
            assert first[j] == i[0] and (w[j, n:] == 0).all(), (n_src, n_dst, j)
            ulp = float(np.spacing(F(np.abs(w64).max())))
            err = np.abs(w[j, :n].astype(np.float64) - w64)
            assert (err[:-1] <= ulp).all(), (n_src, n_dst, j)
            residual = (n - 1) * U * np.abs(w64).max() + max(n - 2, 0) * U * np.abs(w64).sum()
            assert err[-1] <= ulp + residual, (n_src, n_dst, j, err[-1], residual)


@pytest.mark.parametrize("pair", PAIRS)
def test_images_agree_with_the_float64_statement_within_the_derived_bound(pair):
    (W, H), (ow, oh) = pair
    img = _image(W, H)
    for filter in ref.FILTERS:
        got = ref.resample(img, (ow, oh), filter).astype(np.float64)
        want = resample64(img, (ow, oh), filter)
        vmax, bound = 1.0, 0.0
        for n_src, n_dst in ((H, oh), (W, ow)):                      # along v first, then along u
            if n_src == n_dst:
                continue
            w = ref.weights(n_src, n_dst, filter)[1]
            A = float(np.abs(w.astype(np.float64)).sum(axis=1).max())
            bound = bound * A + (w.shape[1] + 2) * U * A * vmax      # the earlier error amplified, plus this pass' own
            vmax = vmax * A
        err = float(np.abs(got - want).max())
        print("%s -> %s %-9s max error %.3g, bound %.3g" % ((W, H), (ow, oh), filter, err, bound))
        assert err <= bound, (filter, err, bound)                    # the clamp is 1-Lipschitz: it widens nothing


def test_box_at_integer_factors_is_the_block_mean():
    img = _image(64, 48)
    for fu, fv in ((2, 2), (4, 3), (8, 6), (1, 2)):
        got = ref.resample(img, (64 // fu, 48 // fv), "box").astype(np.float64)
        mean = img.astype(np.float64).reshape(64 // fu, fu, 48 // fv, fv, 3).mean(axis=(1, 3))
        assert np.abs(got - mean).max() <= ((fu + 2) + (fv + 2)) * U, (fu, fv)
        first, w = ref.weights(48, 48 // fv, "box")
        assert w.shape[1] == fv and (first == fv * np.arange(48 // fv)).all()
        if fv in (2, 4, 8):
            assert (w == F(1.0 / fv)).all()
    first, w = ref.weights(16, 64, "box")                                # enlarging: the nearest sample, weight 1
    assert w.shape[1] == 1 and (w == 1).all() and (first == np.arange(64) // 4).all()


def test_an_axis_of_equal_size_is_a_bit_exact_copy():
    img = _image(48, 40)
    img[3, 5] = (np.nan, -0.0, 7.0)
    for filter in ref.FILTERS:
        same = ref.resample(img, (48, 40), filter)
        assert ((_bits(same) == _bits(img)) | (np.isnan(same) & np.isnan(img))).all()      # both axes: the identity, unclamped
        a = ref.resample(img, (48, 24), filter)                                            # u is a copy: every column is filtered on its own
        for u in (0, 3, 47):
            assert (_bits(a[u]) == _bits(ref.resample(img[u:u + 1], (1, 24), filter)[0])).all()
        b = ref.resample(img, (32, 40), filter)                                            # v is a copy: every row is filtered on its own
        for v in (0, 5, 39):
            assert (_bits(b[:, v]) == _bits(ref.resample(img[:, v:v + 1], (32, 1), filter)[:, 0])).all()
        assert (_bits(a) == _bits(ref.clamp01(ref._pass(img, 1, ref.weights(40, 24, filter))))).all()


@pytest.mark.parametrize("filter", ref.FILTERS)
def test_black_and_clipped_white_stay_exact(filter):
    for (W, H), size in PAIRS + [((128, 64), (16, 8)), ((16, 8), (128, 64))]:
        for value in (0.0, 1.0):
            got = ref.resample(np.full((W, H, 3), value, F), size, filter)
            assert got.shape == size + (3,) and (_bits(got) == _bits(F(value))).all(), ((W, H), size, value)


@pytest.mark.parametrize("pair", PAIRS)
def test_flipping_the_input_flips_the_output_within_the_bound(pair):
    """The taps are added in ascending order whichever way the image lies, and the correction sits on the last tap, so a flipped input meets the
    mirrored weights in another order and with the correction on the other edge: the flip holds to the bound of the float64 comparison (both
    sides are within it of the same exact result, whose flip is exact), not bit for bit.  Along an axis that is a copy it is bit for bit."""
    (W, H), (ow, oh) = pair
    img = _image(W, H, 1)
    for filter in ref.FILTERS:
        plain = ref.resample(img, (ow, oh), filter)
        vmax, bound = 1.0, 0.0
        for n_src, n_dst in ((H, oh), (W, ow)):
            if n_src == n_dst:
                continue
            w = ref.weights(n_src, n_dst, filter)[1]
            A = float(np.abs(w.astype(np.float64)).sum(axis=1).max())
            bound = bound * A + (w.shape[1] + 2) * U * A * vmax
            vmax = vmax * A
        for axis, copy in ((0, ow == W), (1, oh == H)):
            flipped = np.flip(ref.resample(np.ascontiguousarray(np.flip(img, axis)), (ow, oh), filter), axis)
            if copy:
                assert (_bits(flipped) == _bits(plain)).all(), (filter, axis)
            else:
                assert np.abs(flipped.astype(np.float64) - plain).max() <= 2 * bound, (filter, axis)
