"""DE_FLAG_FAST_MATH against the contract kernel by PAIRED samples: N single-sample frames with the flag off and on, same seed, pixels and sample indices.
Only the samples that took another path differ, so the difference D = F - C has a fraction of either frame's variance, and its mean — the flag's bias — is
tested per region of the frame at |z| <= 5 (tests/fast_math_frames.py).  The whole-frame test this joins (tests/test_gpu_round5.py::
test_fast_math_flag_is_statistically_the_same_image) allows 1 %; each view here must reject a stack scaled by 1 +- 1e-2, and what it would still detect is
printed and recorded in profiles/r5_fast_math.md.  Then the special cameras with the flag on."""
import numpy as np
import pytest

import fast_math_frames as ff

pytestmark = pytest.mark.gpu

R_EARTH = 6371e3
N = 128                  # single-sample frames per stack
SIZE = (256, 128)


@pytest.fixture(scope="module")
def Renderer():
    from digital_earth_amd.renderer import Renderer as R
    return R


def _view(Renderer, view, size, seed=5):
    from digital_earth_amd import _native
    heavy = view == "sunset_heavy"
    r = Renderer(size, (0, 1, 0), texture_source="synthetic", texture_size=(2048, 1024), cloud_heavy=heavy, seed=seed)
    if view == "default":
        r.set_fov(0.42)
    elif view == "sunset_heavy":          # limb, terminator and thick cloud in one view
        from digital_earth_amd.earth_viewer import load_config
        load_config("config - sunset hurricane.txt").apply(r)
    elif view == "inside_atmosphere":     # 9 km up on the day side, looking along the atmosphere
        r.set_camera_pos(0.0, 2.0e3, R_EARTH + 9000.0); r.set_look_at(1.0e6, 0.0, R_EARTH + 9000.0); r.set_fov(0.3)
        r.set_sun_angle(1.1); r.set_sun_path_rot(-0.4)
    elif view == "north_pole_down":       # atan2 near (0, 0), asin near 1
        r.set_camera_pos(0.0, R_EARTH + 4.0e5, 0.0); r.set_look_at(0.0, 0.0, 0.0); r.set_up(0.0, 0.0, 1.0)
        r.set_sun_angle(1.1); r.set_sun_path_rot(-0.4)
    elif view == "clamp_sampler":         # the CLAMP instantiation of the fast kernel
        r.set_fov(0.45)
        r.set_flag(_native.DE_FLAG_CLAMP_SAMPLER, True)
    else:
        raise KeyError(view)
    r._push_params()
    r.copy_textures()
    return r


def _stacks(make, n):
    """C[s], F[s]: (n, W, H, 3) single-sample frames s = 0 .. n - 1, flag off and on."""
    out = []
    for fast in (False, True):
        r = make()
        r.set_fast_math(fast)
        frames = []
        for s in range(n):
            r.reset_framebuffer()
            r.set_current_spp(s)
            r.accumulate(1)
            frames.append(r.fetch_hdr())
        assert not fast or r.last_call_info()["variant"] == 6      # every fast call runs render_kernel_v6, whatever its size
        r.close()
        out.append(np.stack(frames))
    return out


@pytest.mark.timeout(300)
@pytest.mark.parametrize("view", ["default", "sunset_heavy", "inside_atmosphere", "north_pole_down", "clamp_sampler"])
def test_flag_moves_samples_not_the_estimate(Renderer, view):
    C, F = _stacks(lambda: _view(Renderer, view, SIZE), N)
    # structure: finite; some samples moved, fewer than the 25 % of the test this joins; every sample keeps its wavelength; an unmoved black sample is black
    assert np.isfinite(C).all() and np.isfinite(F).all()
    moved = ff.moved_mask(C, F)
    lit = (np.abs(C).max(-1) > 0) | (np.abs(F).max(-1) > 0)
    frac = moved.sum() / float(lit.sum())
    worst, n_lit = ff.proportional(C, F)
    print("FASTFRAME %s: N = %d, %d x %d, lit %d, moved %d = %.3f %% of lit; colour proportionality %.2e over %d samples"
          % (view, N, SIZE[0], SIZE[1], lit.sum(), moved.sum(), 100 * frac, worst, n_lit))
    assert lit.sum() > 0.1 * lit.size
    assert 0.0 < frac < 0.25
    assert worst <= 1e-5
    assert (F[~moved & (np.abs(C).max(-1) == 0)] == 0).all()
    # the statistic
    rows = ff.paired_z(C, F)
    regs = ff.regions(moved)
    for (name, n, m, z), mask in zip(rows, [None] + regs):
        print("FASTFRAME %s %s: %d pixel-samples, %d moved, z = %+.2f, detectable delta %s" % (view, name, n, m, z, ff.detectable_delta(C, F, mask)))
    assert rows[0][2] >= ff.MIN_MOVED
    for name, n, m, z in rows:
        assert abs(z) <= ff.Z_MAX, (view, name, z)
    # power: the measured stack scaled by 1 +- 1e-2 is rejected for the whole frame
    yc, yf = ff.luminance(C), ff.luminance(F)
    for s in (1.0, -1.0):
        zs = ff.z_value(yf * (1.0 + s * 1e-2) - yc)
        print("FASTFRAME %s scaled by %+.0e: z = %+.2f" % (view, s * 1e-2, zs))
        assert abs(zs) > ff.Z_MAX, (view, s, zs)


SPECIAL = {
    "centre": dict(pos=(0.0, 0.0, 0.0), look=(1.0, 0.0, 0.0)),
    "inside": dict(pos=(R_EARTH * 0.5, 1000.0, -2000.0), look=(R_EARTH * 2, 0.0, 0.0)),
    "north_pole_down": dict(pos=(0.0, R_EARTH + 4.0e5, 0.0), look=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)),
    "south_axis_up": dict(pos=(0.0, -(R_EARTH + 9.0e3), 0.0), look=(0.0, -(R_EARTH + 1.0e6), 0.0), up=(1.0, 0.0, 0.0)),
    "on_x_axis": dict(pos=(R_EARTH + 2.0e6, 0.0, 0.0), look=(0.0, 0.0, 0.0)),
    "grazing_inside_atmosphere": dict(pos=(R_EARTH + 9000.0, 0.0, 0.0), look=(R_EARTH + 9000.0, 0.0, 1.0e6), fov=0.3),
    "negative_terrain_scale": dict(pos=(-15e6, 0.0, 15e6), look=(0.0, 0.0, 0.0), scale=-8000.0),
    "wide_fov": dict(pos=(R_EARTH + 3.0e5, 1.0e5, 0.0), look=(0.0, 0.0, 0.0), fov=1.5),
    "fixed_wavelength_low": dict(pos=(0.0, 2.0e3, R_EARTH + 1.2e4), look=(1.0e6, 0.0, R_EARTH), fixed=610.0),
    "degenerate": dict(degenerate=True),
}


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", list(SPECIAL))
def test_special_cameras_with_the_flag_on(Renderer, case):
    """The path-tracer cases of tests/test_gpu_parity.py::test_special_cameras_match_the_oracle and its degenerate (all-NaN) camera, 64 x 32 x 2 samples, flag on:
    the frames are finite, the degenerate camera's is all zeros, and the paired statistic holds over the frame wherever at least 500 samples moved.

    Why the fast kernel's loops end where the contract's do (de_stages.h):
      * sphere_trace ends on `cnt >= 250` whatever its other two tests see: no leaf value matters.
      * the gas and cloud tracking steps end on `!(t < tmax)`, true for a NaN t.  t advances by -de_log_unit(u) / sigma: it needs de_log_unit(u) < 0 and finite for
        every draw u > 0 (t never falls back and never turns NaN on a finite ray) and de_log_unit(0) = -inf (t = +inf ends the segment) —
        test_gpu_fast_math_leaves.py::test_log_of_every_draw asserts both over all 2^24 draws.
      * a NaN or inside-the-planet camera reaches the loops through length_nr = de_sqrt_nr and de_rcp_nr: de_sqrt_nr of NaN, of a negative discriminant and of
        -inf must be NaN (so that `len > lower && len < upper` is false and no map or bound cell is addressed from a NaN point, and rsi's miss stays a miss),
        de_rcp_nr(NaN) NaN — test_classes_on_special_values[sqrt_nr], [rcp_nr] hold the classes of exactly these inputs to the contract's.
      * every other leaf (exp, sin, cos, atan2, asin, pow) shapes weights, directions and map coordinates only; a NaN there is a NaN radiance, which write_contrib
        zeroes, or a NaN direction, which the rules above end.
      * the vertex loop is bounded by its own counter."""
    W, H = 64, 32
    cfg = SPECIAL[case]

    def make():
        r = Renderer((W, H), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=4)
        r.copy_textures()
        if cfg.get("degenerate"):
            r.set_look_at(*[float(x) for x in r.camera_pos[None]])
            return r
        r.set_camera_pos(*cfg["pos"]); r.set_look_at(*cfg["look"]); r.set_up(*cfg.get("up", (0.0, 1.0, 0.0)))
        if "fov" in cfg: r.set_fov(cfg["fov"])
        if "scale" in cfg: r.land_height_scale = cfg["scale"]
        if "fixed" in cfg: r.set_fixed_wavelength(cfg["fixed"])
        r.set_sun_angle(1.1); r.set_sun_path_rot(-0.4)
        r._push_params()
        return r

    C, F = _stacks(make, 2)
    assert np.isfinite(F).all() and np.isfinite(C).all()
    moved = ff.moved_mask(C, F)
    z = ff.z_value(ff.luminance(F) - ff.luminance(C))
    print("FASTSPECIAL %s: lit %d, moved %d, z = %+.2f" % (case, (np.abs(F).max(-1) > 0).sum(), moved.sum(), z))
    if cfg.get("degenerate"):
        assert (F == 0).all() and (C == 0).all()
    if moved.sum() >= ff.MIN_MOVED:
        assert abs(z) <= ff.Z_MAX, (case, z)
