"""The numpy restatement of the video frame output (tests/video_ref.py, the yardstick of tests/test_gpu_video.py) held to an independent float64
statement of the H.273 equations (tests/video_f64.py) and to closed forms.  No GPU.

Against float64, for truncate and round: wherever the float64 value ahead of the quantiser lies farther than 1e-3 code from its decision boundary (an
integer for truncation, an integer plus a half for rounding) the codes are equal — f32 rounding through this chain (a dozen operations on values of at
most 1023, ulp 6e-5, relative error 6e-8 each) stays orders below 1e-3 code — elsewhere they differ by at most 1; and the excluded share is at most
1 %: the images are random colours, for which a 2e-3-wide band around the boundaries holds 0.2 % of the samples."""
import numpy as np
import pytest

import video_f64
import video_ref as vr

F = np.float32


def _random_image(W, H, seed):
    rng = np.random.default_rng(seed)
    img = rng.uniform(-0.1, 1.1, (W, H, 3)).astype(F)      # a tenth of the values clip at either end
    img[0, 0] = (np.nan, -0.0, np.inf)
    return img


def _flat(W, H, rgb):
    return np.broadcast_to(np.asarray(rgb, F), (W, H, 3)).copy()


# ---------------------------------------------------------------- against float64
@pytest.mark.parametrize("format", ("i420", "i010"))
@pytest.mark.parametrize("matrix", vr.MATRICES)
@pytest.mark.parametrize("range_", vr.RANGES)
@pytest.mark.parametrize("siting", vr.SITINGS)
def test_restatement_against_float64(format, matrix, range_, siting):
    W, H = 22, 14
    img = _random_image(W, H, 7 + vr.MATRICES.index(matrix))
    want = video_f64.values(img, vr.bits(format), matrix, range_ == "full", siting)
    for mode, offset in (("truncate", 0.0), ("round", 0.5)):
        got = vr.codes(img, format, matrix, range_, siting, mode)
        excluded = total = 0
        for g, w in zip(got, want):
            code = np.floor(w + offset).astype(np.int64)
            frac = (w + offset) - np.floor(w + offset)
            near = (frac < 1e-3) | (frac > 1.0 - 1e-3)
            assert (g[~near] == code[~near]).all(), (mode, np.argwhere((g != code) & ~near)[:4].tolist())
            assert np.abs(g - code).max() <= 1
            excluded += int(near.sum()); total += near.size
        print("%s %s %s %s %s: excluded %d of %d" % (format, matrix, range_, siting, mode, excluded, total))
        assert excluded <= 0.01 * total, (excluded, total)


# ---------------------------------------------------------------- closed forms
@pytest.mark.parametrize("format", vr.FORMATS)
@pytest.mark.parametrize("mode", vr.MODES)
def test_black_and_white_are_exact_in_every_mode(format, mode):
    k = 4 if vr.bits(format) == 10 else 1
    top = 1023 if vr.bits(format) == 10 else 255
    for matrix in vr.MATRICES:
        c = vr.consts(format, matrix, "limited")
        assert F(F(c["kr"] + c["kb"]) + c["kg"]) == F(1.0)      # white has Y = 1 exactly
        for siting in vr.SITINGS:
            for phase in (0, 3):
                slack = 1 if mode == "dither" else 0          # neutral chroma is a mid-range code: the dither moves it by one LSB like any other; the end codes never move
                y, cb, cr = vr.codes(_flat(8, 6, (0, 0, 0)), format, matrix, "limited", siting, mode, 9, phase)
                assert (y == 16 * k).all() and np.abs(cb - 128 * k).max() <= slack and np.abs(cr - 128 * k).max() <= slack
                y, cb, cr = vr.codes(_flat(8, 6, (1, 1, 1)), format, matrix, "limited", siting, mode, 9, phase)
                assert (y == 235 * k).all() and np.abs(cb - 128 * k).max() <= slack and np.abs(cr - 128 * k).max() <= slack
                y, cb, cr = vr.codes(_flat(8, 6, (0, 0, 0)), format, matrix, "full", siting, mode, 9, phase)
                assert (y == 0).all()
                y, cb, cr = vr.codes(_flat(8, 6, (2.0, np.inf, 1.0)), format, matrix, "full", siting, mode, 9, phase)
                assert (y == top).all()


def test_full_range_chroma_reaches_both_ends():
    for format, top in (("i420", 255), ("i010", 1023)):
        y, cb, cr = vr.codes(_flat(4, 4, (0, 0, 1)), format, "bt709", "full", "center", "round")      # blue: Cb = +0.5
        assert (cb == top).all()
        y, cb, cr = vr.codes(_flat(4, 4, (1, 1, 0)), format, "bt709", "full", "center", "truncate")   # yellow: Cb = -0.5 -> 0.5 code, truncated
        assert (cb == 0).all()
        y, cb, cr = vr.codes(_flat(4, 4, (1, 0, 0)), format, "bt709", "full", "center", "round")      # red: Cr = +0.5
        assert (cr == top).all()


def test_bt709_primaries_give_the_standards_codes():
    # 8-bit limited BT.709: the colour-bar values of the 100 % primaries (Rec. ITU-R BT.709 with H.273's quantisation, rounded)
    table = {(1, 0, 0): (63, 102, 240), (0, 1, 0): (173, 42, 26), (0, 0, 1): (32, 240, 118),
             (1, 1, 0): (219, 16, 138), (0, 1, 1): (188, 154, 16), (1, 0, 1): (78, 214, 230)}
    for rgb, (Y, Cb, Cr) in table.items():
        for siting in vr.SITINGS:
            y, cb, cr = vr.codes(_flat(6, 4, rgb), "i420", "bt709", "limited", siting, "round")
            assert (y == Y).all() and (cb == Cb).all() and (cr == Cr).all(), (rgb, siting, y[0, 0], cb[0, 0], cr[0, 0])
            y, cb, cr = vr.codes(_flat(6, 4, rgb), "i010", "bt709", "limited", siting, "round")
            kr, kb = 0.2126, 0.0722
            ey = kr * rgb[0] + (1 - kr - kb) * rgb[1] + kb * rgb[2]
            want = (int(np.floor(4 * (219 * ey + 16) + 0.5)), int(np.floor(4 * (224 * 0.5 * (rgb[2] - ey) / (1 - kb) + 128) + 0.5)), int(np.floor(4 * (224 * 0.5 * (rgb[0] - ey) / (1 - kr) + 128) + 0.5)))
            assert (int(y[0, 0]), int(cb[0, 0]), int(cr[0, 0])) == want, (rgb, siting)


@pytest.mark.parametrize("siting", vr.SITINGS)
def test_a_flat_image_gives_flat_chroma(siting):
    rng = np.random.default_rng(5)
    for rgb in rng.uniform(0, 1, (6, 3)):
        vals, _ = vr.prequant(_flat(10, 6, rgb), "i010", "bt2020", "limited", siting)
        for p in vals:
            assert (p == p[0, 0]).all()                       # the dyadic weights add to 1 without rounding: bit-equal, not merely close
        ref = vr.prequant(_flat(10, 6, rgb), "i010", "bt2020", "limited", "center")[0]
        assert all((a == b).all() for a, b in zip(vals, ref))


@pytest.mark.parametrize("column", (0, 1, 4, 5, 10, 11))
def test_a_chroma_impulse_lands_where_the_siting_puts_it(column):
    """One blue column on black: Cb is an impulse of height 0.5 in column `column` (W = 12, so 0 and W - 1 are among them), constant down the rows.  The
    chroma samples must hold it with the weights the siting defines — in steps of 224 * 4 * 0.5 = 448 codes at 10 bits, exactly representable."""
    W, H = 12, 6
    img = np.zeros((W, H, 3), F)
    img[column, :, 2] = 1.0
    base = vr.codes(np.zeros((W, H, 3), F), "i010", "bt709", "limited", "center", "round")[1]
    i = column // 2
    for siting in vr.SITINGS:
        cb = vr.codes(img, "i010", "bt709", "limited", siting, "round")[1] - base
        assert (cb == cb[0]).all()                            # the same in every chroma row
        want = np.zeros(W // 2)
        if siting == "center":
            want[i] = 0.5                                     # the mean of columns 2i and 2i + 1
        elif column % 2 == 0:
            want[i] = 0.5                                     # [1 2 1] / 4 centred on it ...
            if column == 0:
                want[i] += 0.25                               # ... and the tap at -1 repeats column 0
        else:
            want[i] = 0.25                                    # the right-hand tap of sample i ...
            if i + 1 < W // 2:
                want[i + 1] = 0.25                            # ... and the left-hand tap of sample i + 1 (none behind column W - 1)
        assert (cb[0] == np.round(want * 448).astype(np.int64)).all(), (siting, column, cb[0].tolist())


def test_a_chroma_row_impulse_and_the_top_edge():
    """The same down the rows: one blue output row r.  LEFT and CENTER take the mean of rows 2j and 2j + 1; TOPLEFT [1 2 1] / 4 centred on 2j, row -1 repeating row 0."""
    W, H = 6, 12
    base = vr.codes(np.zeros((W, H, 3), F), "i010", "bt709", "limited", "center", "round")[1]
    for r in (0, 1, 4, 5, 10, 11):
        img = np.zeros((W, H, 3), F)
        img[:, H - 1 - r, 2] = 1.0
        j = r // 2
        for siting in vr.SITINGS:
            cb = vr.codes(img, "i010", "bt709", "limited", siting, "round")[1] - base
            want = np.zeros(H // 2)
            if siting != "topleft":
                want[j] = 0.5
            elif r % 2 == 0:
                want[j] = 0.5 + (0.25 if r == 0 else 0.0)
            else:
                want[j] = 0.25
                if j + 1 < H // 2:
                    want[j + 1] = 0.25
            assert (cb[:, 0] == np.round(want * 448).astype(np.int64)).all() and (cb == cb[:, :1]).all(), (siting, r)


def test_layouts_are_the_same_codes():
    img = _random_image(18, 10, 3)
    for mode in vr.MODES:
        i010, p010 = vr.pack(img, "i010", mode=mode, seed=4, phase=2), vr.pack(img, "p010", mode=mode, seed=4, phase=2)
        W, H = 18, 10
        a, b = i010.view("<u2"), p010.view("<u2")
        assert (b[:W * H] == a[:W * H] << 6).all()                                    # P010 = I010 << 6 ...
        n = (W // 2) * (H // 2)
        assert (b[W * H:].reshape(-1, 2)[:, 0] == a[W * H:W * H + n] << 6).all() and (b[W * H:].reshape(-1, 2)[:, 1] == a[W * H + n:] << 6).all()
        i420, nv12 = vr.pack(img, "i420", mode=mode, seed=4, phase=2), vr.pack(img, "nv12", mode=mode, seed=4, phase=2)
        assert (nv12[:W * H] == i420[:W * H]).all()
        assert (nv12[W * H:].reshape(-1, 2)[:, 0] == i420[W * H:W * H + n]).all() and (nv12[W * H:].reshape(-1, 2)[:, 1] == i420[W * H + n:]).all()   # ... NV12 = I420 interleaved
        for f, frame in (("i010", i010), ("p010", p010), ("i420", i420), ("nv12", nv12)):
            assert frame.dtype == np.uint8 and frame.size == W * H * 3 // 2 * (2 if vr.bits(f) == 10 else 1)
            assert all((x == y).all() for x, y in zip(vr.planes(frame, W, H, f), vr.codes(img, f, mode=mode, seed=4, phase=2)))


# ---------------------------------------------------------------- dither
def test_dither_is_unbiased_where_rounding_is_not_and_keeps_the_end_codes():
    """A grey ramp over a few codes in steps of 1/64 code: the mean over 64 phases follows it; rounding is off by up to half a code."""
    W, H = 64, 8
    grey = (np.arange(W * H, dtype=np.float64).reshape(W, H) / (W * H) * 4.0 + 100.0 - 16.0) / 219.0       # Y codes 100 ... 104
    img = np.repeat(grey[..., None], 3, axis=2).astype(F)
    truth = video_f64.values(img, 8, "bt709", False, "left")[0]
    rounded = vr.codes(img, "i420", mode="round")[0]
    mean = np.mean([vr.codes(img, "i420", mode="dither", seed=1, phase=p)[0] for p in range(64)], axis=0)
    err_round, err_dither = np.abs(rounded - truth).mean(), np.abs(mean - truth).mean()
    print("mean |error|: round %.4f, dither over 64 phases %.4f" % (err_round, err_dither))
    assert err_dither < err_round and err_dither < 0.1
    for format in ("i420", "i010"):
        for range_ in vr.RANGES:
            c = vr.consts(format, "bt709", range_)
            for phase in range(8):
                lo = vr.codes(_flat(8, 8, (0, 0, 0)), format, "bt709", range_, "left", "dither", 2, phase)
                hi = vr.codes(_flat(8, 8, (1, 1, 1)), format, "bt709", range_, "left", "dither", 2, phase)
                assert (lo[0] == int(c["ylo"])).all() and (hi[0] == int(c["yhi"])).all()
                blue = vr.codes(_flat(8, 8, (0, 0, 1)), format, "bt709", range_, "left", "dither", 2, phase)
                assert (blue[1] == int(c["chi"])).all()          # the highest legal chroma code stays exact too
