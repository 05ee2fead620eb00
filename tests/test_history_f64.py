"""The numpy float32 restatement of the history reprojection (tests/history_ref.py, which the device is held to bit for bit) against an independent
float64 statement of DESIGN.md §13 (tests/history_f64.py), from 2 m above the ground to 21 000 km out, without a GPU.

The restatement used to form the world point first, q = (cam + dir t) - cam_h: P is rounded at planet scale (0.25 - 0.5 m), the difference cancels,
and q keeps that absolute error however short the ray.  From 21 000 km, where every earlier test stood, that costs nothing; at 2 m it moved the
reprojected position of these cases by up to 2.0 px and at 100 m by 0.10 px (3.9e5 S and 2.1e4 S in the unit below; 1.0 px from the oblique 100 m
position, where all three coordinates are of planet size), so that a still camera did not map a pixel onto itself.  With q = (cam - cam_h) + dir t every term is rounded relative to itself.

Budgets (tests/history_cases.py counts them): the position of every conditioned pixel in front of the history's camera may differ by N S with S = 2^-24 max(W, H, H / (2 fov_h)) px and N = 59, the number of f32
roundings of steps 2 - 4 on the way to xo (fu 6, fv 4, the ray's sum 12, its normalisation 10, cam - cam_h 3, dir t 3, their sum 3, z 5, the dot with
du_h 5, the quotient 1, xo's own chain 7), which is larger than four times the worst measured over this sweep (4.1 S on land, 4.2 S at infinity);
r by 47 roundings of |cam - cam_h| + |t| (measured 4.2); out by G N S + 26 x 2^-24 max(|m|, |h|) wherever every
tap that a floor() within the position budget would read is valid (the still camera: the 3 x 3 history pixels about the pixel), and by the derived
(4 G + |h - m|) N S / B only where one of them is invalid or outside the image.  Decisions (have, the four taps' validity, x0, y0)
are compared where the float64 statement says no threshold lies within these budgets; that mask may exclude at most 1 % of any case's pixels.  The
"identical" history camera puts every xo on an integer on purpose: there floor() is anyone's, so its decisions are compared through the continuous
quantities only (position, B, out), and the 1 % cap holds for its other conditions."""
import itertools

import numpy as np
import pytest

import history_cases as hc
import history_f64 as h64
import history_ref as hr

GROUPS = list(itertools.product(hc.SIZES, hc.ALTITUDES, hc.FOVS))
_F32 = {}


def _pair(key):
    """(case, the f32 restatement's (out, details)) — computed once."""
    x = hc.case(*key)
    if key not in _F32:
        _F32[key] = hr.blend(x["m"], x["n"], x["dist"], x["cam"], x["hist"], x["hist_d"], x["hcam"], details=True)
    return x, _F32[key]


def _conditioned(f, history):
    ill = f["ill"]
    return ~(ill["depth"] | ill["z"] | ill["s"] | ill["B"]) if history == "identical" else ~ill["any"]


def _position_error(f, rp):
    with np.errstate(all="ignore"):
        return np.maximum(np.abs(rp["xo"].astype(np.float64) - f["xo"]), np.abs(rp["yo"].astype(np.float64) - f["yo"]))


@pytest.mark.parametrize("size,altitude,fov", GROUPS)
def test_positions_and_decisions_match_float64(size, altitude, fov):
    worst = dict(land=0.0, sky=0.0, infinity=0.0, r=0.0, excluded=0.0)
    for view, history in itertools.product(hc.VIEWS, hc.HISTORY_CAMERAS):
        x, (_, rp) = _pair((size, altitude, fov, view, history))
        f = x["f64"]
        what = (size, altitude, fov, view, history)
        cond = _conditioned(f, history)
        S = f["pos"] / hc.N_POS
        e = _position_error(f, rp)
        # every conditioned pixel in front of the history's camera, inside its image or not
        front = cond & (f["z"] > 0)
        land = front & f["land"]
        sky = front & ~f["land"] & ~f["at_infinity"]
        infinity = front & f["at_infinity"]
        assert (e[land] <= f["pos"]).all(), (what, float(e[land].max() / S))
        assert (e[infinity] <= f["pos"]).all(), (what, float(e[infinity].max() / S))
        # the tangent point: s's own rounding moves it along the ray, which a translated history camera sees as parallax (hc.sky_parallax)
        assert (e[sky] <= (f["pos"] + hc.sky_parallax(f))[sky]).all(), what
        if history in ("identical", "yaw 1.5 px", "turned around"):
            assert (hc.sky_parallax(f) == 0).all()
        # r, which the surface test reads on land
        on_land = cond & f["land"]
        er = np.abs(rp["r"].astype(np.float64) - f["r"])
        assert (er[on_land] <= f["len"][on_land]).all(), what
        # decisions
        assert (rp["have"] == f["have"])[cond].all(), what
        if history != "identical":
            assert (rp["valid"] == f["valid"])[:, cond].all(), what
            assert (rp["x0"] == f["x0"])[cond].all() and (rp["y0"] == f["y0"])[cond].all(), what
        else:
            reach = f["z"] > 0
            assert f["ill"]["grid"][reach].all()                               # a still camera lands on the grid: the reason for the exemption
        # the cap on exclusions: a condition on the cases, not a measurement
        excluded = float((~cond).mean())
        assert excluded <= 0.01, (what, excluded)
        if size != (16, 8):
            assert int((cond & (f["at_infinity"] if view == "up" else f["land"])).sum()) >= 100, what      # looking up there is no land: the pixels at infinity
        for k, v in (("land", e[land] / S), ("sky", (e - hc.sky_parallax(f))[sky] / S), ("infinity", e[infinity] / S), ("r", (er / (f["len"] / hc.N_LEN))[on_land])):
            worst[k] = max(worst[k], float(v.max()) if v.size else 0.0)
        worst["excluded"] = max(worst["excluded"], excluded)
    print("worst over %s: position %.2f S on land, %.2f S at the tangent point (beyond the parallax), %.2f S at infinity; r %.2f roundings; excluded %.4f"
          % ((size, altitude, fov), worst["land"], worst["sky"], worst["infinity"], worst["r"], worst["excluded"]))
    # N is the larger of the count and four times the measured worst: what history_cases.py records as measured is what this sweep gives
    assert max(worst["land"], worst["sky"], worst["infinity"]) <= hc.MEASURED_POS and worst["r"] <= hc.MEASURED_LEN


@pytest.mark.parametrize("size,altitude,fov", GROUPS)
def test_blend_matches_float64(size, altitude, fov):
    seen = dict(blended=0, first=0, none=0, partial=0)
    for view, history in itertools.product(hc.VIEWS, hc.HISTORY_CAMERAS):
        x, (out, rp) = _pair((size, altitude, fov, view, history))
        f = x["f64"]
        what = (size, altitude, fov, view, history)
        cond = _conditioned(f, history)
        bound = hc.blend_bound(x)
        err = np.abs(out[..., :3].astype(np.float64) - f["out"])
        assert (err[cond] <= bound[cond]).all(), (what, float((err[cond] / np.maximum(bound[cond], 1e-300)).max()))
        # Wout = n + min(Wh, max_history) B: B moves only where a tap is missing, by at most 4 N S
        full = f["full"]
        weight = min(float(x["hist"][0, 0, 3]), hr.DEFAULTS["max_history"])
        wb = np.where(full, 0.0, 4.0 * f["pos"] * weight) + hc.K_BLEND * h64.EPS * f["Wout"]
        ew = np.abs(out[..., 3].astype(np.float64) - f["Wout"])
        assert (ew[cond] <= wb[cond]).all(), (what, float((ew[cond] / wb[cond]).max()))
        none = cond & ~f["have"]
        assert (out[none][:, :3].view(np.uint32) == x["m"][none].view(np.uint32)).all() and (out[none][:, 3] == x["n"][none]).all(), what
        seen["blended"] += int((cond & f["have"] & (x["n"] > 0)).sum())
        seen["first"] += int((cond & f["have"] & (x["n"] == 0)).sum())
        seen["none"] += int(none.sum())
        seen["partial"] += int((cond & f["have"] & ~full).sum())
    assert min(seen.values()) > 0, seen


@pytest.mark.parametrize("size", hc.SIZES)
@pytest.mark.parametrize("altitude", ["2 m", "100 m", "100 m, oblique"])
@pytest.mark.parametrize("fov", hc.FOVS)
def test_a_still_low_camera_maps_every_pixel_onto_itself(size, altitude, fov):
    """tests/test_history_ref.py's property where it used to fail: the former expression gave up to 2.0 px at 2 m and 0.10 px at 100 m."""
    W, H = size
    u = np.arange(W)[:, None] + np.zeros((1, H))
    v = np.arange(H)[None, :] + np.zeros((W, 1))
    for view in hc.VIEWS:
        x, (_, rp) = _pair((size, altitude, fov, view, "identical"))
        f = x["f64"]
        cond = _conditioned(f, "identical")
        assert cond.mean() >= 0.99
        assert (np.abs(rp["xo"] - u)[cond] <= f["pos"]).all() and (np.abs(rp["yo"] - v)[cond] <= f["pos"]).all(), (view, float(np.abs(rp["xo"] - u)[cond].max()))
        assert rp["have"][cond].all()
        inner = np.zeros((W, H), bool)
        inner[1:-1, 1:-1] = True
        assert (np.abs(rp["B"].astype(np.float64) - 1.0)[cond & inner] <= f["B_bound"]).all(), view


def test_the_views_hold_what_they_are_chosen_for():
    for altitude, fov in itertools.product(hc.ALTITUDES, hc.FOVS):
        f = hc.case((80, 56), altitude, fov, "horizon", "identical")["f64"]
        assert 0.1 < f["land"].mean() < 0.9, (altitude, fov)                                                  # land and sky
        if fov == 0.05:                       # and the limb's tangent points (s > 0) between them: from 2 m at fov 0.4 that band is thinner than a pixel
            assert (~f["land"] & ~f["at_infinity"]).any(), altitude
        assert hc.case((80, 56), altitude, fov, "up", "identical")["f64"]["at_infinity"].all()                # s <= 0: only the direction reprojects
        if altitude != "21 000 km":
            assert hc.case((80, 56), altitude, fov, "down", "identical")["f64"]["land"].all()
        assert not hc.case((80, 56), altitude, fov, "horizon", "turned around")["f64"]["have"].any()
