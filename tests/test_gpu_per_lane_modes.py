"""The per-lane kernel body (render_kernel.hip: per_lane_body) has three modes — 0 accumulate, 1 accumulate + work counters, 2 trace one sample
per pixel — times two samplers.  ray_march_kernel is that body around the ray marcher; the legacy library's render_kernel (kernel variant 1,
tests/legacy/test_gpu_per_lane_v1.py) is the same body around the per-lane path tracer.  What is held here needs no oracle: the modes agree
with each other.  Image 32 x 16 (8 tiles, 2 workgroups), synthetic maps 1024 x 512, fov 0.4."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 32, 16


def make_renderer(clamp, marcher, variant=None):
    from digital_earth_amd import _native
    from digital_earth_amd.renderer import Renderer
    r = Renderer((W, H), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512))
    r.set_fov(0.4)
    r.set_flag(_native.DE_FLAG_CLAMP_SAMPLER, clamp)
    if marcher:
        r.set_integrator("ray_marcher")
    if variant is not None:
        r.set_kernel_variant(variant)
    return r


def _frame(r, counters, calls):
    r.enable_counters(counters)
    r.reset_framebuffer()
    for spp in calls:
        r.accumulate(spp)
    return r.fetch_hdr().view(np.uint32)


def check_counters_do_not_change_the_frame(r):
    """MODE 1 against MODE 0 at 2 spp."""
    assert (_frame(r, True, [2]) == _frame(r, False, [2])).all()


def check_launch_shape_does_not_change_the_frame(r):
    """The kernel read-modify-writes the HDR buffer itself: three launches of one sample are one launch of three."""
    assert (_frame(r, False, [1, 1, 1]) == _frame(r, False, [3])).all()


def check_counters_agree_with_the_trace(r):
    """MODE 1 against MODE 2 at 1 spp: every pixel's draws and vertices, summed."""
    _frame(r, True, [1])
    cnt = r.counters()
    trace = r.debug_samples(0).astype(np.float64)
    print(cnt, trace[..., 2].sum(), trace[..., 3].sum())
    assert cnt["samples"] == W * H
    assert cnt["rng_draws"] == int(trace[..., 2].sum())
    assert cnt["vertices"] == int(trace[..., 3].sum())


def check_trace_leaves_the_frame_alone(r):
    """MODE 2 stores nothing into the frame."""
    before = _frame(r, False, [2])
    r.debug_samples(0)
    assert (r.fetch_hdr().view(np.uint32) == before).all()


CHECKS = [check_counters_do_not_change_the_frame, check_launch_shape_does_not_change_the_frame, check_counters_agree_with_the_trace,
          check_trace_leaves_the_frame_alone]


@pytest.fixture(scope="module", params=[False, True], ids=["repeat", "clamp"])
def marcher(request):
    return make_renderer(request.param, marcher=True)


@pytest.mark.parametrize("check", CHECKS, ids=lambda f: f.__name__[len("check_"):])
def test_ray_marcher(marcher, check):
    check(marcher)
    assert marcher.last_call_info()["variant"] == 0      # the ray marcher's kernel ran
