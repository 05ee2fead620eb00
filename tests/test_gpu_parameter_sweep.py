"""The render kernels against the CPU oracle on the seeded parameter sweep of tests/sweep_cases.py (48 configurations that combine camera height,
position, view, sun, field of view, terrain scale, wavelength mode, sampler, integrator, map set and launch shape; tests/test_sweep_cases.py shows on
the oracle alone what they reach).  Every case, bit for bit: the HDR frame of render_kernel_v2, of render_kernel_v6 and of the automatic choice (the
ray marcher's one kernel for its cases), the per-sample trace of both samples, the work counters; and the displayed image within the display path's
bound.  A failure prints the case, which `sweep_cases.apply` replays alone."""
import numpy as np
import pytest

import sweep_cases as sc
from helpers import bits_equal_fraction, make_oracle, rel_l2

pytestmark = pytest.mark.gpu

W, H = sc.FRAME
CASES = sc.cases()


@pytest.fixture(scope="module")
def scenes():
    """One Renderer per (map sizes, map seed, cloud variant) with the maps it generated, made on first use and kept for the module."""
    from digital_earth_amd.renderer import Renderer
    made = {}

    def scene(case):
        key = sc.map_key(case)
        if key not in made:
            sizes = dict(enumerate(sc.MAP_SIZES[case["map_sizes"]]))
            r = Renderer((W, H), (0, 1, 0), texture_source="synthetic", texture_size=sizes, cloud_heavy=case["cloud_heavy"], synth_seed=case["map_seed"])
            r.copy_textures()
            made[key] = (r, [r.download_texture(s) for s in range(7)])
        return made[key]
    yield scene
    made.clear()


def _same_bits(a, b):
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _launch(r, case):
    r.reset_framebuffer()
    for n in case["calls"]:
        r.accumulate(n)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kernels_match_the_oracle(scenes, lut_arrays, case):
    r, texels = scenes(case)
    r.seed = case["seed"]
    r.enable_counters(False)
    sc.apply(case, r._params)
    r._push_params()
    o = make_oracle(W, H, lut_arrays, texels, r._params)
    for n in case["calls"]:
        o.accumulate(n, case["seed"])
    want = o.fetch_hdr()
    assert np.isfinite(want).all()
    # ---- the HDR frame, every kernel that can render it
    for variant in ((4,) if case["marcher"] else (2, 6, 4)):
        r.set_kernel_variant(variant)
        _launch(r, case)
        got = r.fetch_hdr()
        ran = r.last_call_info()["variant"]
        if case["marcher"] or variant != 4:      # forcing a kernel at this frame size is supported; 0 = ray_march_kernel
            assert ran == (0 if case["marcher"] else variant), (variant, ran)
        same = bits_equal_fraction(got, want)
        if same != 1.0:
            print("variant %d (ran %d): bit-identical %.6f, rel L2 %.3e\n%r" % (variant, ran, same, rel_l2(got, want), case))
        assert np.isfinite(got).all(), (case["id"], variant)
        assert same == 1.0, (case["id"], variant)
    # ---- the displayed image of that accumulation (the automatic choice's)
    assert np.abs(r.fetch_image() - o.fetch_image()).max() <= 1e-5, case["id"]
    # ---- the per-sample trace: radiance, wavelength, draw count, vertex count
    for k in range(sc.SPP):
        dg, dc = r.debug_samples(k), o.debug_samples(case["seed"], k)
        for field, name in enumerate(("radiance", "wavelength", "draws", "vertices")):
            bad = ~_same_bits(dg[..., field], dc[..., field])
            assert not bad.any(), (case["id"], k, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    # ---- the work counters
    r.enable_counters(True)
    _launch(r, case)
    g, c = r.counters(), o.counters()
    r.enable_counters(False)
    for name in ("samples", "tracking_steps", "vertices", "rng_draws", "taps_rgb8"):
        assert g[name] == c[name], (case["id"], name, g, c)
    # the GPU skips the cloud taps the reference multiplies by zero and the sphere-trace steps of escaped rays (test_counters_match_oracle)
    assert g["taps_r8"] <= c["taps_r8"] and g["sphere_steps"] <= c["sphere_steps"], (case["id"], g, c)
    assert bits_equal_fraction(r.fetch_hdr(), want) == 1.0, (case["id"], "counting launch")
