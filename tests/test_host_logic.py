"""Host-side logic that needs no GPU: camera math, config round trip, tile partition."""
import os
import numpy as np

from digital_earth_amd import parallel
from digital_earth_amd.earth_viewer import Camera, Config, load_config, np_rotate_matrix, np_normalize


def test_rotate_matrix_is_a_rotation():
    m = np_rotate_matrix(np.array([0.0, 1.0, 0.0]), 0.3)[:3, :3]
    assert np.allclose(m @ m.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(m) - 1) < 1e-12
    v = m @ np.array([1.0, 0, 0])
    assert np.allclose(v, [np.cos(0.3), 0, -np.sin(0.3)])   # counter-clockwise about +y (lib/math_utils.py:83-102)


def test_camera_defaults_and_motion():
    c = Camera(None, (0, 1, 0))
    assert (c.position == [-15000000., 0.0, 15000000.]).all() and (c.look_at == 0).all()   # earth_viewer.py:26-27
    assert np.allclose(c.target_dir, np_normalize(np.array([1.0, 0, -1.0])))
    d0 = np.linalg.norm(c.look_at - c.position)
    c.rotate(0.01, 0.0)
    assert abs(np.linalg.norm(c.look_at - c.position) - d0) < 1e-3     # rotation keeps the view distance
    p0 = c.position.copy()
    c.move(c.target_dir, 0.1)
    assert np.linalg.norm(c.position - p0) > 0
    assert c.update_camera(0.1) is True       # earth_viewer.py:146-155: reports the change once
    assert c.update_camera(0.1) is False


def test_config_round_trip(tmp_path):
    a = load_config("config - Apollo 11.txt")
    p = tmp_path / "config.txt"
    a.write(str(p))
    b = load_config(str(p))
    for k in ("fov", "aspect_scale", "exposure", "selected_crf", "gamma", "sun_angle", "sun_path_rot"):
        assert getattr(a, k) == getattr(b, k)
    assert (a.position == b.position).all() and (a.look_at == b.look_at).all() and (a.up == b.up).all()
    assert len(open(p).read().splitlines()) == 10


def test_presets_parse_to_the_files_tokens():
    """The product's 10-line preset parser against the raw tokens of the reference's three preset files."""
    import os
    from digital_earth_amd import luts
    for name in ("config - florida.txt", "config - sunset hurricane.txt", "config - Apollo 11.txt"):
        with open(os.path.join(luts.CONFIG_DIR, name)) as f:
            want = [float(t) for t in f.read().split()]
        assert len(want) == 16
        c = load_config(name)
        got = list(c.position) + list(c.look_at) + list(c.up) + [c.fov, c.aspect_scale, c.exposure, c.selected_crf, c.gamma,
                                                                  c.sun_angle, c.sun_path_rot]
        assert got == want, name


def test_tile_partition_masks():
    W, H = 1920, 1080
    for world in (1, 2, 4, 8):
        masks = [parallel.owned_pixel_mask(W, H, r, world) for r in range(world)]
        total = np.sum(masks, axis=0)
        assert (total == 1).all()                                      # every pixel has exactly one owner
        counts = parallel.tiles_per_rank(W, H, world)
        assert counts.sum() == (W // 8) * (H // 8) and counts.max() - counts.min() <= 135   # balanced to within one tile column
        for r in range(world):
            assert masks[r].sum() == counts[r] * 64
    # ownership rule used by the kernel: 8x8 tile (tx, ty) -> (tx + ty) % world
    m = parallel.owned_pixel_mask(64, 32, 1, 4)
    assert m[8, 0] and not m[0, 0] and m[0, 8] and m[7 + 8 * 5, 7]


def test_image_orientation_matches_taichi_imread(tmp_path):
    """ti.tools.imread gives [x][y] with y up (renderer.py:63-93): texel row 0 must be the image's bottom row (v = 0 = south)."""
    from PIL import Image
    from digital_earth_amd import textures as T
    img = np.zeros((4, 6, 3), np.uint8)
    img[0, :, 0] = 200          # top row of the picture = north
    img[3, :, 0] = 10           # bottom row = south
    p = tmp_path / "m.png"
    Image.fromarray(img).save(str(p))
    t = T.load_image_texels(str(p), 1)
    assert t.shape == (4, 6, 1) and (t[0, :, 0] == 10).all() and (t[3, :, 0] == 200).all()
    assert T.load_image_texels(str(p), 3).shape == (4, 6, 3)


def _bench_args(argv):
    import importlib
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    old = sys.argv
    sys.argv = ["bench.py"] + list(argv)
    try:
        return bench, bench.parse()
    finally:
        sys.argv = old


def test_bench_names_the_baseline_configs():
    """`bench.py --config cfgN` sets the workload from BASELINE.json's wording and the line's metric names it (a cfg4 run used to print
    the cfg2 metric string).  The table is held to BASELINE.json itself: size, sample count and preset of every config appear in its text."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    texts = json.load(open(os.path.join(root, "BASELINE.json")))["configs"]
    bench, a = _bench_args([])
    assert (a.width, a.height, a.spp, a.preset, a.config_name) == (1920, 1080, 64, None, "cfg2")      # the default run IS cfg2
    for name, c in bench.CONFIGS.items():
        text = texts[c["index"]]
        assert "%d×%d" % (c["width"], c["height"]) in text and "%d spp" % c["spp"] in text
        if c["preset"]:
            assert c["preset"] in text and os.path.exists(os.path.join(root, "digital_earth_amd", "data", "configs", c["preset"]))
        assert c["cloud_heavy"] == ("cloud-heavy" in text) and (c["progressive"] > 0) == ("progressive" in text)
        _, a = _bench_args(["--config", name])
        assert (a.width, a.height, a.spp, a.preset, bool(a.cloud_heavy), a.progressive, a.config_name) == \
               (c["width"], c["height"], c["spp"], c["preset"], c["cloud_heavy"], c["progressive"], name)
        m = bench.metric_name(a.width, a.height, a.spp, a.preset, a.cloud_heavy, a.progressive)
        assert "%dx%d, %d spp" % (c["width"], c["height"], c["spp"]) in m and (not c["preset"] or c["preset"] in m)
    # cfg5's film curve is taken by name and the name is one of the shipped curves
    from digital_earth_amd import luts
    assert bench.CONFIGS["cfg5"]["crf_name"] in luts.load_crfs()[0]
    # flags that spell a config are recognised; anything else is not a BASELINE config and says so in its metric
    _, a = _bench_args(["--preset", "config - florida.txt", "--spp", "256"])
    assert a.config_name == "cfg3"
    _, a = _bench_args(["--spp", "16", "--width", "256", "--height", "128"])
    assert a.config_name is None and "256x128, 16 spp" in bench.metric_name(a.width, a.height, a.spp, a.preset, a.cloud_heavy, a.progressive)
    # the sparse tiles of the full-sample-count oracle checks: about half a million paths each, never more than a million
    from oracle import oracle_binding as ob
    for name, (first, stride) in bench.SPARSE_CHECK.items():
        c = bench.CONFIGS[name]
        mask = ob.Oracle.strided_mask(c["width"], c["height"], first, stride)
        paths = int(mask.sum()) * c["spp"]
        assert 0 <= first < stride and 2e5 < paths < 1.1e6, (name, paths)
        # spread over the frame: tiles in every quarter of the image
        w2, h2 = c["width"] // 2, c["height"] // 2
        assert all(q.any() for q in (mask[:w2, :h2], mask[w2:, :h2], mask[:w2, h2:], mask[w2:, h2:])), name


def test_bench_dump_outputs_are_bounded_and_reproducible(tmp_path):
    """`bench.py --dump-outputs DIR` (plain runs are lean: `--full` is off by default): whole frames where they fit, above the limit the same
    seeded sample of pixels from run to run and from array to array, float32, never more than DUMP_LIMIT_BYTES in all."""
    import numpy as np
    bench, a = _bench_args(["--dump-outputs", str(tmp_path)])
    assert a.dump_outputs == str(tmp_path) and a.full is False and _bench_args(["--full"])[1].full is True

    class Frame:
        def __init__(self, w, h):
            self.hdr = np.random.default_rng(1).random((w, h, 3), dtype=np.float32)
            self.r = self

        def fetch_hdr(self):
            return self.hdr

        def fetch_image(self):
            return self.hdr / 2

    def dumped(frame, d):
        bench.write_outputs(str(d), frame)
        return {k: np.load(d / (k + ".npy")) for k in ("hdr", "image")}

    whole = dumped(Frame(1920, 1080), tmp_path / "cfg2")                  # 49.8 MB: written whole
    assert whole["hdr"].shape == (1920, 1080, 3) and (whole["image"] == whole["hdr"] / 2).all()
    big = Frame(3840, 2160)                                                 # cfg4: 199 MB, sampled
    one, two = dumped(big, tmp_path / "a"), dumped(big, tmp_path / "b")
    assert one["hdr"].dtype == np.float32 and one["hdr"].ndim == 2 and one["hdr"].shape[1] == 3
    assert sum(x.nbytes for x in one.values()) <= bench.DUMP_LIMIT_BYTES
    assert one["hdr"].shape[0] > 0.9 * bench.DUMP_LIMIT_BYTES / 24
    assert all((one[k] == two[k]).all() for k in one) and (one["image"] == one["hdr"] / 2).all()
