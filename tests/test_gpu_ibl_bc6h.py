"""The BC6H stage on the GPU (include/digital_earth_ibl_bc6h.h): the encoder alone, the bake with the compressed file out, and end to end
behind render_environment and build_ibl, each byte for byte against the numpy restatement (tests/bc6h_ref.py over digital_earth_amd/bc6h.py)."""
import io
import os
import re

import numpy as np
import pytest

import bc6h_ref as br
from digital_earth_amd import bc6h

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_STATE = -1, -4
N = 16
SCENE = dict(texture_source="synthetic", texture_size=(1024, 512))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BODY = open(os.path.join(ROOT, "digital_earth_amd", "csrc", "bc6h_body.h")).read()
THREADS = int(re.search(r"#define BC6H_THREADS (\d+)", _BODY).group(1))
Q0_GROUP = int(re.search(r"#define BC6H_Q0_GROUP_BLOCKS (\d+)", _BODY).group(1))
Q1_GROUP = THREADS // int(re.search(r"#define BC6H_Q1_LANES (\d+)", _BODY).group(1))
# 4 x 4, 8 x 8, 5 x 7, and one image past a workgroup's share and no multiple of it in each launch shape: 132 x 36 = 33 x 9 = 297 blocks (256 a group at
# quality 0: two groups, the second 41 blocks; 8 a group at quality 1: 38 groups, the last 1 block)
SHAPES = [(4, 4), (8, 8), (5, 7), (132, 36)]


@pytest.fixture(scope="module")
def ctx():
    from digital_earth_amd import renderer
    r = renderer.Renderer((N, N), (0, 1, 0), **SCENE)
    r.copy_textures()
    yield r
    r.close()


def test_the_large_shape_leaves_a_partial_workgroup_in_both_launch_shapes():
    blocks = 33 * 9
    assert blocks > Q0_GROUP and blocks % Q0_GROUP and blocks > Q1_GROUP and blocks % Q1_GROUP


@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("w,h", SHAPES)
def test_the_encoder_equals_the_restatement(ctx, w, h, quality):
    img = br.test_image(w, h, seed=w)
    got = ctx.debug_bc6h_encode(img, quality)
    want = br.encode(img, quality)
    bad = [k for k in range(len(want) // 16) if got[16 * k:16 * k + 16] != want[16 * k:16 * k + 16]]
    assert len(got) == len(want) and not bad, (len(bad), bad[:8])
    if (w, h) == (132, 36) and quality == 1:
        assert len(set(bc6h.block_modes(got, 297).tolist())) >= 3      # the image does reach the two-region modes


def _faces(seed):
    rng = np.random.default_rng(2900 + seed)
    v = (rng.random((6, N, N, 3)) * 40).astype(np.float32)
    v[:, :, N // 2:] *= np.float32(0.05)
    v[4, N // 2 + 1, N // 3] = np.float32(1e7)
    return v


@pytest.mark.parametrize("quality", [0, 1])
@pytest.mark.parametrize("shape", [dict(edge=8, levels=4, samples=8, supersample=1), dict(edge=32, levels=3, samples=8, supersample=1)], ids=["E8-L4", "E32-L3"])
def test_the_bake_with_the_compressed_file_out(ctx, shape, quality):
    from PIL import Image
    sh, levels, halves, data = ctx.debug_ibl_bc6h(_faces(shape["edge"]), quality=quality, **shape)
    sh2, levels2, _ = ctx.debug_ibl(_faces(shape["edge"]), **shape)
    for a, b in zip(levels, levels2):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))              # the same bake
    for a, h in zip(levels, halves):
        assert np.array_equal(bc6h.to_half(a), h.astype(np.int64))                # the half levels are the source the blocks encode
    assert data == bc6h.write([h.astype(np.int64) for h in halves], quality)      # byte for byte, header included
    back, info = bc6h.read(data)
    assert info == dict(edge=shape["edge"], levels=shape["levels"])
    for l, h in enumerate(halves):
        for face in range(6):
            want = bc6h.decode_blocks(bc6h.encode_blocks(h[face], quality), h.shape[1], h.shape[1])
            assert np.array_equal(back[l][face], want)
    img = Image.open(io.BytesIO(data))
    assert img.size == (shape["edge"], shape["edge"]) and img.mode == "RGB"
    first = back[0][0].view(np.float16).astype(np.float64)
    assert np.abs(np.clip(np.floor(first * 255), 0, 255) - np.asarray(img).astype(np.int64)).max() <= 1      # Pillow's truncated interpolation: tests/test_bc6h_ref.py


def test_end_to_end_and_refusals(ctx):
    from digital_earth_amd import dds
    r = ctx
    r.set_camera_pos(-5.5e6, 1.0e6, 5.5e6)
    r.set_look_at(0.0, 0.0, 0.0)
    r.set_up(0.0, 1.0, 0.0)
    r.vignette_strength = 0.0
    shape = dict(edge=16, levels=5, samples=8, supersample=2)
    try:
        assert r.ibl_bc6h["on"] is False and r.ibl_bc6h["quality"] == 0      # the defaults
        r.set_panorama((64, 32), apron=1, supersample=2)
        r.set_ibl(**shape)
        r.set_ibl_bc6h(True, quality=1)
        assert r.ibl_bc6h == dict(on=True, quality=1, file_bytes=148 + 96 * (16 + 4 + 1 + 1 + 1))
        for bad in (dict(quality=2), dict(quality=-1)):
            with pytest.raises(Exception) as e:
                r.set_ibl_bc6h(True, **bad)
            assert e.value.code == ERR_INVALID and r.ibl_bc6h["quality"] == 1
        with pytest.raises(Exception) as e:
            r.fetch_ibl_bc6h_dds()
        assert e.value.code == ERR_STATE                                    # before the build
        r.render_environment(2)
        r.build_ibl()
        levels = [np.stack([r.fetch_ibl_face(l, face) for face in range(6)]) for l in range(5)]
        plain_on = r.fetch_ibl_dds()
        for quality in (1, 0):
            r.set_ibl_bc6h(True, quality=quality)
            data = r.fetch_ibl_bc6h_dds()
            assert len(data) == r.ibl_bc6h["file_bytes"] and data == bc6h.write(levels, quality)
            assert r.fetch_ibl_bc6h_dds() == data                           # the kept blocks
        assert max(level.max() for level in levels) > 0
        r.set_ibl_bc6h(False)
        with pytest.raises(Exception) as e:
            r.fetch_ibl_bc6h_dds()
        assert e.value.code == ERR_STATE                                    # the stage off
        assert r.fetch_ibl_dds() == plain_on == dds.write(levels, "half")   # the half file is what it was, on or off
        r.set_ibl_bc6h(True)
        r.set_ibl(**shape)
        with pytest.raises(Exception) as e:
            r.fetch_ibl_bc6h_dds()
        assert e.value.code == ERR_STATE                                    # new IBL settings drop the product
        r.build_ibl()
        assert r.fetch_ibl_bc6h_dds() == bc6h.write(levels, 0)
    finally:
        r.set_ibl_bc6h(False)
        r.set_panorama((64, 32), on=False)
