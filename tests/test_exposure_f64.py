"""The restatement of the auto-exposure meter (tests/exposure_f64.py) checked on its own, without a GPU: the bin edges, 8 bins in every octave and a
monotone bin index, centres strictly inside their bins, the trimming worked by hand on five pixels (with the hi == lo rule at N = 1), the EV update."""
import numpy as np

import exposure_f64 as ae


def _f32(x):
    return np.float32(x)


def test_bin_edges_and_range_ends():
    lo = _f32(2.0 ** -24)
    b, below, clipped = ae.bin_of(np.array([lo, np.nextafter(lo, _f32(0)), _f32(2.0 ** 8), np.nextafter(_f32(2.0 ** 8), _f32(0)), _f32(0), _f32(-1), _f32(np.nan), _f32(np.inf),
                                            _f32(1e-45), _f32(1.0)], np.float32))
    assert b.tolist() == [0, -1, 255, 255, -1, -1, -1, 255, -1, 24 * 8]
    assert below.tolist() == [False, True, False, False, True, True, True, False, True, False]
    assert clipped.tolist() == [False, False, True, False, False, False, False, True, False, False]


def test_every_octave_holds_8_bins_and_the_index_is_monotone():
    edges = ae.bin_edges()
    assert edges[0] == 2.0 ** -24 and edges[-1] == 2.0 ** 8 and (np.diff(edges) > 0).all()
    e32 = edges.astype(np.float32)
    assert (e32.astype(np.float64) == edges).all()            # the edges are f32 numbers
    b, below, _ = ae.bin_of(e32[:-1])
    assert b.tolist() == list(range(256)) and not below.any()  # an edge opens its bin ...
    b, _, _ = ae.bin_of(np.nextafter(e32[1:], np.float32(0)))
    assert b.tolist() == list(range(256))                      # ... and the number just under the next edge is still inside
    for octave in range(-24, 8):
        inside = [k for k in range(256) if 2.0 ** octave <= edges[k] < 2.0 ** (octave + 1)]
        assert len(inside) == 8 and inside == list(range((octave + 24) * 8, (octave + 24) * 8 + 8))
    rng = np.random.default_rng(1)
    y = np.sort(np.exp2(rng.uniform(-30, 10, 20000)).astype(np.float32))
    b, _, _ = ae.bin_of(y)
    assert (np.diff(b) >= 0).all()


def test_centres_lie_strictly_inside_their_bins():
    c, edges = ae.centres(), ae.bin_edges()
    assert c.shape == (256,)
    assert (np.exp2(c) > edges[:-1]).all() and (np.exp2(c) < edges[1:]).all()
    assert c[24 * 8] == np.log2(1.0 + 0.5 / 8.0)             # [1, 1.125)
    assert abs(np.exp2(c[0]) - 2.0 ** -24 * 1.0625) < 1e-22


def test_luminance_order_of_operations():
    m = np.array([[0.3, 0.5, 0.7]], np.float32)
    want = (np.float32(0.2126) * m[0, 0] + np.float32(0.7152) * m[0, 1]) + np.float32(0.0722) * m[0, 2]
    assert ae.luminance(m)[0] == want and ae.luminance(m).dtype == np.float32


def test_meter_divides_like_the_display_and_respects_the_region():
    W, H = 8, 4
    sums = np.zeros((W, H, 3), np.float32)
    sums[..., 1] = 7.0 * 0.5          # mean g = 0.5 at 7 samples: Y = 0.7152f * 0.5f, octave -2
    sums[2, 1] = 0.0                  # one black pixel
    sums[3, 2, 1] = 7.0 * 1000.0      # one clipped pixel
    m = ae.meter(sums, 7)
    y = np.float32(0.7152) * np.float32(0.5)
    k = int(ae.bin_of(np.array([y], np.float32))[0][0])
    assert m["metered"] == W * H - 1 and m["below"] == 1 and m["clipped"] == 1
    assert m["histogram"][k] == W * H - 2 and m["histogram"][255] == 1
    m = ae.meter(sums, 7, region=(0, 0, 3, 2))                # holds the black pixel, not the clipped one
    assert m["metered"] == 5 and m["below"] == 1 and m["clipped"] == 0
    per_pixel = np.full((W, H), 7, np.int32)
    per_pixel[3, 2] = 7000                                    # the clipped pixel's own count brings it back to g = 1
    m = ae.meter(sums, per_pixel)
    assert m["clipped"] == 0 and m["metered"] == W * H - 1


def test_trimming_by_hand_on_five_pixels():
    c = ae.centres()
    h = np.zeros(256, np.uint32)
    h[10], h[20], h[30] = 1, 3, 1                             # ranks: 0 | 1 2 3 | 4
    # 0.2 .. 0.8 as f32: lo = floor(0.2f * 5) = 1, hi = floor(0.8f * 5) = 4: the three pixels of bin 20
    assert np.float64(np.float32(0.2)) * 5 > 1.0 and np.float64(np.float32(0.8)) * 5 > 4.0
    assert ae.trimmed_mean(h, 0.2, 0.8) == c[20]
    # 0 .. 1: everything
    assert ae.trimmed_mean(h, 0.0, 1.0) == ((1.0 * c[10] + 3.0 * c[20]) + 1.0 * c[30]) / 5.0
    # 0.5 .. 1: lo = 2, hi = 5: two of bin 20, one of bin 30
    assert ae.trimmed_mean(h, 0.5, 1.0) == (2.0 * c[20] + 1.0 * c[30]) / 3.0
    # lo = floor(0.45f * 5) = 2 = hi = floor(0.55f * 5): hi becomes 3, the median pixel
    assert ae.trimmed_mean(h, 0.45, 0.55) == c[20]
    # N = 1: lo = hi = 0 -> the one pixel
    one = np.zeros(256, np.uint32)
    one[77] = 1
    assert ae.trimmed_mean(one, 0.10, 0.95) == c[77]
    assert ae.trimmed_mean(np.zeros(256, np.uint32), 0.10, 0.95) is None


def test_ev_update_clamp_adaptation_and_black_frames():
    c = ae.centres()
    h = np.zeros(256, np.uint32)
    h[100] = 10
    m = ae.Meter()
    r = m.update(h, manual_exposure=3.0)
    want = np.log2(np.float64(np.float32(0.18))) - c[100]
    assert r["valid"] and r["ev_target"] == want and r["ev"] == float(np.float32(want)) and r["mean_log2"] == c[100]
    # the clamp bites, the compensation shifts
    assert ae.Meter(ev_range=(-1.0, 2.0)).update(h)["ev"] == 2.0
    assert ae.Meter(compensation=1.5).update(h)["ev_target"] == want + 1.5
    # adaptation: the first display jumps, the next ones ease; the state is the f32 that was used
    m = ae.Meter(adapt=0.25)
    e0 = m.update(h)["ev"]
    assert e0 == float(np.float32(want))
    h2 = np.zeros(256, np.uint32)
    h2[140] = 10
    t2 = np.log2(np.float64(np.float32(0.18))) - c[140]
    e1 = m.update(h2)["ev"]
    assert e1 == float(np.float32(e0 + 0.25 * (t2 - e0)))
    # black: the EV stays and no state is made from it
    black = np.zeros(256, np.uint32)
    r = m.update(black)
    assert not r["valid"] and r["ev"] == e1
    m.clear()
    r = m.update(black, manual_exposure=3.25)
    assert not r["valid"] and r["ev"] == 3.25
    assert m.update(h2)["ev"] == float(np.float32(t2))        # still the first valid metering: it jumps


def test_ulps():
    assert ae.ulps_f32(1.0, 1.0) == 0.0
    assert ae.ulps_f32(1.0, np.nextafter(np.float32(1.0), np.float32(2.0))) == 1.0
