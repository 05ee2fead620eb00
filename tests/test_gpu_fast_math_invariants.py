"""The launch invariants pinned for the contract kernel, on the DE_FLAG_FAST_MATH compile of render_kernel_v6 (csrc/de_fast.hip): a separate compile of the
persistent LDS-queue scheduler, with other register pressure and timing.  Every comparison is bit for bit against the fast kernel itself: a path's bits do not
depend on the run, the launch shape, the tile partition, the tail chain, the adaptive frame's rounds or the call's size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KW = dict(texture_source="synthetic", texture_size=(1024, 512))


@pytest.fixture(scope="module")
def Renderer():
    from digital_earth_amd.renderer import Renderer as R
    return R


def _fast(Renderer, size=(128, 64), seed=11, fov=0.42, **kw):
    r = Renderer(size, (0, 1, 0), seed=seed, **dict(KW, **kw))
    r.set_fov(fov)
    r.set_fast_math(True)
    r.copy_textures()
    return r


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.timeout(120)
def test_same_frame_twice_in_fresh_contexts(Renderer):
    frames = []
    for _ in range(2):
        r = _fast(Renderer)
        r.accumulate(4)
        assert r.last_call_info()["variant"] == 6
        frames.append(r.fetch_hdr())
        r.close()
    assert frames[0].max() > 0 and (_bits(frames[0]) == _bits(frames[1])).all()


@pytest.mark.timeout(120)
def test_progressive_launches_and_tile_ranks(Renderer):
    """accumulate(4) == 4 x accumulate(); 1 rank == 2 and 8 virtual tile ranks."""
    r = _fast(Renderer)
    r.accumulate(4)
    full = r.fetch_hdr()
    r.reset_framebuffer()
    for _ in range(4):
        r.accumulate()
    assert r.current_spp == 4 and (_bits(r.fetch_hdr()) == _bits(full)).all()
    for world in (2, 8):
        r.reset_framebuffer()
        for rank in range(world):
            r.set_tile_partition(rank, world)
            r.set_current_spp(0)
            r.accumulate(4)
        r.set_tile_partition(0, 1)
        assert (_bits(r.fetch_hdr()) == _bits(full)).all(), world
    r.close()


@pytest.mark.timeout(300)
def test_tail_chain_with_calls_in_flight(Renderer):
    """The tail forced on through set_tuning as tests/test_gpu_round5.py::test_tail_chain_with_calls_in_flight_and_partitions does, one and two levels, several
    calls in flight on the launch slots, a tile partition: the frames of the chain equal the no-tail frames."""
    def frames(levels, export0, grid0, alone):
        r = _fast(Renderer)
        t = r.tuning()
        t.v6_tail_levels = levels; t.v6_tail_export[0] = export0; t.v6_tail_grid[0] = grid0
        t.v6_tail_export[1] = 24; t.v6_tail_grid[1] = 4; t.v6_tail_min_paths = 0
        t.v6_tail_when_alone = alone
        r.set_tuning(t)
        out = []
        for spp in (3, 1, 4, 2, 1, 3):      # six calls, nothing waits in between
            r.accumulate(spp)
        assert r.last_call_info()["variant"] == 6
        out.append(r.fetch_hdr())
        r.reset_framebuffer(); r.set_tile_partition(2, 5); r.accumulate(3); r.accumulate(2)
        out.append(r.fetch_hdr())
        r.close()
        return out

    ref = frames(0, 96, 64, 1)
    assert ref[0].max() > 0 and ref[1].max() > 0
    for levels, export0, grid0, alone in ((1, 128, 64, 0), (1, 128, 64, 1), (2, 400, 128, 1)):
        for a, b in zip(ref, frames(levels, export0, grid0, alone)):
            assert (_bits(a) == _bits(b)).all(), (levels, export0, grid0, alone)


@pytest.mark.timeout(300)
def test_adaptive_tiles_equal_uniform_fast_frames(Renderer):
    """tests/test_gpu_adaptive.py's core property, one size, one view: every tile of an adaptive frame, at the count it stopped at, holds the bits of a uniform
    frame of that count."""
    r = _fast(Renderer, texture_size=(2048, 1024))
    for tau in (0.4, 0.25, 0.15, 0.1, 0.06, 0.04, 0.025, 0.015, 0.01):
        r.reset_framebuffer()
        r.render_adaptive(tau, 32, min_spp=4, round_spp=4)
        counts, hdr = r.tile_spp(), r.fetch_hdr()
        values = np.unique(counts)
        if len(values) >= 3 and values[-1] == 32 and values[0] < 32:
            break
    else:
        pytest.fail("no threshold spreads the tile counts")
    for n in values:
        r.reset_framebuffer()
        r.accumulate(int(n))
        m = np.repeat(np.repeat(counts == n, 8, axis=0), 8, axis=1)
        assert (_bits(hdr)[m] == _bits(r.fetch_hdr())[m]).all(), (tau, n)
    r.close()


@pytest.mark.timeout(120)
def test_a_call_below_4096_paths(Renderer):
    """A call of 2048 paths (one of 8 tile ranks of a 128 x 64 x 2 call) runs render_kernel_v6 under the flag — de_launch.h sends every fast call there,
    whatever its size — and gives the bits those pixels get in the larger call."""
    from digital_earth_amd import parallel
    r = _fast(Renderer)
    r.accumulate(2)
    full = r.fetch_hdr()
    r.reset_framebuffer()
    r.set_tile_partition(3, 8)
    r.accumulate(2)
    assert r.last_call_info()["variant"] == 6
    part = r.fetch_hdr()
    own = parallel.owned_pixel_mask(128, 64, 3, 8)
    assert own.sum() == 1024 and (part[~own] == 0).all() and part[own].max() > 0
    assert (_bits(part)[own] == _bits(full)[own]).all()
    r.close()
