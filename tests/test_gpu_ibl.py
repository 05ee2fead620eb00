"""The IBL bake on the GPU (include/digital_earth_ibl.h) against tests/ibl_ref.py, bit for bit: every face of every level, the nine SH
coefficients and the DDS file, through de_debug_ibl on random faces with a sun, and end to end behind render_environment at N = 16.  The device's
square root (Renderer.debug_math 8) is handed to the restatement.  Shapes: E = 16 is one partial 16 x 16 tile per face down to edge 1; E = 64 has four
tiles per axis at level 0 and two at level 1, so a swapped tile decode leaves a tile unwritten; E = 32, L = 6, K = 64 clamps the level of detail at
both ends and drops samples (tests/test_ibl_ref.py checks in numpy that it does)."""
import numpy as np
import pytest

import ibl_ref as ir
from digital_earth_amd import dds

pytestmark = pytest.mark.gpu

F = np.float32
ERR_INVALID, ERR_STATE = -1, -4
N = 16
SCENE = dict(texture_source="synthetic", texture_size=(1024, 512))
_f = np.array([2.0, -1.0, 2.0]) / 3.0
_u = np.array([1.0, 2.0, 0.0]) / np.sqrt(5.0)
_u = _u - _f * (_u @ _f)
_u /= np.linalg.norm(_u)
OBLIQUE = np.stack([np.cross(_f, _u), _u, _f])
SHAPES = [dict(edge=16, levels=5, samples=8, supersample=1), dict(edge=64, levels=4, samples=16, supersample=1),
          dict(edge=64, levels=4, samples=16, supersample=3), dict(edge=32, levels=6, samples=64, supersample=2)]


@pytest.fixture(scope="module")
def ctx():
    from digital_earth_amd import renderer
    r = renderer.Renderer((N, N), (0, 1, 0), **SCENE)
    r.copy_textures()
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist(), got[diff][:4], want[diff][:4])


def sun_faces(seed):
    """Values up to 1e4 and one texel at 1e7, a "sun"."""
    rng = np.random.default_rng(2800 + seed)
    v = (rng.random((6, N, N, 3)) * 1e4).astype(F)
    v[4, N // 2 + 1, N // 3] = F(1e7)
    return v


def _check(r, faces, apron, basis, pixel_type, **shape):
    sqrt = lambda x: r.debug_math(8, x)
    sh, levels, data = r.debug_ibl(faces, apron=apron, basis=basis, pixel_type=pixel_type, **shape)
    want_sh, want, _ = ir.bake(faces, apron=apron, basis=basis, sqrt=sqrt, **shape)
    assert len(levels) == shape["levels"]
    for l, (g, w) in enumerate(zip(levels, want)):
        for face in range(6):
            _same(g[face], w[face], "level %d face %d" % (l, face))
    _same(sh, want_sh, "sh")
    assert data == dds.write(levels, pixel_type), "the DDS file"
    back, info = dds.read(data)
    assert info == dict(edge=shape["edge"], levels=shape["levels"], pixel_type=pixel_type)
    return levels


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "E%d-L%d-K%d-S%d" % (s["edge"], s["levels"], s["samples"], s["supersample"]))
@pytest.mark.parametrize("apron", [1, 4])
def test_debug_bake_equals_the_restatement(ctx, shape, apron):
    held = ctx.ibl
    _check(ctx, sun_faces(apron), apron, OBLIQUE if apron == 4 else None, "half" if apron == 1 else "float", **shape)
    assert ctx.ibl == held      # the debug entry point leaves the context alone


@pytest.mark.parametrize("c", [0.0, 0.3, 70000.0])
def test_a_constant_survives_the_device(ctx, c):
    faces = np.full((6, N, N, 3), F(c), F)
    for S in (1, 3, 4):
        sh, levels, data = ctx.debug_ibl(faces, edge=16, levels=5, samples=8, supersample=S, pixel_type="half")
        for level in levels:
            assert (level == F(c)).all()
        half = np.frombuffer(data[dds.HEADER_BYTES:], np.uint16).reshape(-1, 4)
        assert (half[:, :3] == {0.0: 0, 0.3: int(np.float16(0.3).view(np.uint16)), 70000.0: 0x7BFF}[c]).all() and (half[:, 3] == 0x3C00).all()


def _state(r):
    pano = r.panorama
    pano["basis"] = pano["basis"].tobytes()
    return r.ibl, pano, str(r.environment), [r.fetch_environment_face(k).tobytes() for k in r.environment["captured"]]


def test_end_to_end_and_refusals(ctx):
    r = ctx
    r.set_camera_pos(-5.5e6, 1.0e6, 5.5e6)
    r.set_look_at(0.0, 0.0, 0.0)
    r.set_up(0.0, 1.0, 0.0)
    r.vignette_strength = 0.0
    shape = dict(edge=16, levels=5, samples=8, supersample=2)
    try:
        # the stage off
        r.set_panorama((64, 32), on=False)
        r.set_ibl(**shape)
        before = _state(r)
        with pytest.raises(Exception) as e:
            r.build_ibl()
        assert e.value.code == ERR_STATE and _state(r) == before
        with pytest.raises(Exception) as e:
            r.fetch_ibl_sh()
        assert e.value.code == ERR_STATE
        # five faces held
        r.set_panorama((64, 32), apron=1, supersample=2, basis=OBLIQUE)
        r.reset_framebuffer()
        r.accumulate(1)
        for face in range(5):
            r.capture_environment_face(face)
        before = _state(r)
        with pytest.raises(Exception) as e:
            r.build_ibl()
        assert e.value.code == ERR_STATE and _state(r) == before
        # settings out of range: refused, nothing changes (the payload limit itself cannot be reached inside the ranges: tests/test_ibl_abi.py)
        for bad in (dict(edge=2048), dict(edge=1024, levels=12), dict(samples=12), dict(pixel_type="float", edge=24)):
            with pytest.raises(Exception) as e:
                r.set_ibl(**bad)
            assert e.value.code == ERR_INVALID and _state(r) == before
        # all six
        r.render_environment(2, basis=OBLIQUE)
        exr_before, rgbe_before = r.fetch_exr(), r.fetch_rgbe()
        faces = np.stack([r.fetch_environment_face(k) for k in range(6)])
        sqrt = lambda x: r.debug_math(8, x)
        want_sh, want, _ = ir.bake(faces, apron=1, basis=r.panorama["basis"], sqrt=sqrt, **shape)
        for pixel_type in ("half", "float"):
            r.set_ibl(pixel_type=pixel_type, **shape)
            with pytest.raises(Exception) as e:
                r.fetch_ibl_dds()
            assert e.value.code == ERR_STATE      # new settings drop the product
            r.build_ibl()
            levels = [np.stack([r.fetch_ibl_face(l, face) for face in range(6)]) for l in range(shape["levels"])]
            for l in range(shape["levels"]):
                _same(levels[l], want[l], "level %d" % l)
            _same(r.fetch_ibl_sh(), want_sh, "sh")
            data = r.fetch_ibl_dds()
            assert len(data) == r.ibl["file_bytes"] and data == dds.write(levels, pixel_type)
            back, info = dds.read(data)
            assert info["pixel_type"] == pixel_type and info["edge"] == 16 and info["levels"] == 5
            if pixel_type == "float":
                for l in range(5):
                    _same(back[l][..., :3], levels[l])
        assert max(level.max() for level in levels) > 0      # the frame is not empty
        for bad in ((5, 0), (-1, 0), (0, 6)):
            with pytest.raises(Exception) as e:
                r.fetch_ibl_face(*bad)
            assert e.value.code == ERR_INVALID
        # the other outputs of the same panorama are what they were
        assert r.fetch_exr() == exr_before and r.fetch_rgbe() == rgbe_before
    finally:
        r.set_panorama((64, 32), on=False)
        r.set_exr()
