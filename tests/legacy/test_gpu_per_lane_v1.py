"""tests/test_gpu_per_lane_modes.py once more for kernel variant 1: the legacy library's render_kernel is the per-lane kernel body
(render_kernel.hip: per_lane_body) around the per-lane path tracer (legacy/render_kernel_v1.hip)."""
import pytest

pytest.register_assert_rewrite("test_gpu_per_lane_modes")
import test_gpu_per_lane_modes as modes      # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.legacy_quick]


@pytest.fixture(scope="module", params=[False, True], ids=["repeat", "clamp"])
def per_lane(request):
    return modes.make_renderer(request.param, marcher=False, variant=1)


@pytest.mark.parametrize("check", modes.CHECKS, ids=lambda f: f.__name__[len("check_"):])
def test_per_lane_path_tracer(per_lane, check):
    check(per_lane)
    assert per_lane.last_call_info()["variant"] == 1      # the per-lane loops ran
