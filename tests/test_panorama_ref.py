"""The panorama stage's restatement (tests/panorama_ref.py) held to an independent float64 statement of its geometry, without a GPU:
the resampler inverts the renderer's own camera, picks the face the float64 direction picks, keeps constants exactly, and the float64 sphere of the
orientation test stays under that test's cap; the shapes of more than one tile that the GPU tests run reach what they are there for; and the resampled
IMAGE of faces with a linear content equals the float64 closed form at every pixel, which holds the tap addressing to something not written from the
header."""
import numpy as np
import pytest

import panorama_ref as ref

F = np.float32
N = 16
ROUND_TRIP = [((64, 32), "equirect", 180.0), ((32, 32), "fisheye", 180.0), ((32, 32), "fisheye", 360.0)]
# an oblique orthonormal frame (rows r, u, f = the renderer's right, up, forward: r = f x u), exact in float64 up to rounding
_f = np.array([2.0, -1.0, 2.0]) / 3.0
_u = np.array([1.0, 2.0, 0.0]) / np.sqrt(5.0)
_u = _u - _f * (_u @ _f)
_u /= np.linalg.norm(_u)
OBLIQUE = np.stack([np.cross(_f, _u), _u, _f])


def _centres(size):
    w, h = size
    return np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5, indexing="ij")


@pytest.mark.parametrize("apron", (1, 4))
@pytest.mark.parametrize("case", ROUND_TRIP)
@pytest.mark.parametrize("basis", (None, OBLIQUE))
def test_round_trip_through_the_renderers_camera(case, apron, basis):
    """Every pixel centre: direction -> (face, X, Y) by the float32 restatement; the renderer's cast (get_cast_dir, the jitter replaced by the
    fractional position) through that face's camera of the header's table at (X, Y) gives the direction back within 1e-5.  The cast's own 1e-5
    offset (8e-5 of a pixel at N = 16) is dropped in the stage by definition, and so in the float64 cast."""
    size, projection, aperture = case
    x, y = _centres(size)
    want, inside = ref.f64_direction(x, y, size, projection, aperture, basis)
    k = ref.consts(N, apron, aperture, basis)
    cr, cu, cf, outside = ref.sub_direction(size, projection, 1, 0, 0, k)
    assert (outside == ~inside).all()
    face, X, Y = ref.locate(cr, cu, cf, N, k)
    assert X[inside].min() >= apron - 0.5 - 1e-3 and X[inside].max() <= N - apron - 0.5 + 1e-3      # inside the inner 90°: every tap the face's own
    assert Y[inside].min() >= apron - 0.5 - 1e-3 and Y[inside].max() <= N - apron - 0.5 + 1e-3
    worst = 0.0
    for f in range(6):
        sel = inside & (face == f)
        if not sel.any():
            continue
        look, up, fov = ref.f64_face_camera(f, N, apron, basis)
        got = ref.f64_cast_dir(look, up, fov, N, X[sel].astype(np.float64), Y[sel].astype(np.float64))
        worst = max(worst, float(np.abs(got - want[sel]).max()))
    print("round trip %s apron %d: worst component error %.3e" % (case, apron, worst))
    assert worst <= 1e-5
    assert len(np.unique(face[inside])) == (6 if projection == "equirect" or aperture == 360.0 else 5)


@pytest.mark.parametrize("case", ROUND_TRIP)
def test_face_identity(case):
    """Faces filled with their own index come out, at S = 1, as exactly the index of the float64 major axis, but for pixels whose float64 direction
    has its two largest magnitudes within 1e-5 of each other; those are counted and stay under 2 % of the frame (the float64 statement alone first)."""
    size, projection, aperture = case
    x, y = _centres(size)
    d, inside = ref.f64_direction(x, y, size, projection, aperture)
    want, gap = ref.f64_major_axis(d)
    near = inside & (gap <= 1e-5)
    share = near.sum() / float(near.size)
    print("face identity %s: %d near-tie pixels, %.3f %% of the frame" % (case, int(near.sum()), 100.0 * share))
    assert share < 0.02                                            # the float64 statement alone
    faces = np.broadcast_to(np.arange(6, dtype=F)[:, None, None, None], (6, N, N, 3))
    got = ref.panorama(faces, size, projection, aperture, 1, 1)
    check = inside & ~near
    assert (got[check] == want[check][:, None].astype(F)).all()
    assert (got[~inside] == 0).all()
    assert len(np.unique(got[check])) >= 5                         # the faces are told apart: not one value everywhere


@pytest.mark.parametrize("case", [((64, 32), "equirect", 180.0), ((48, 24), "equirect", 180.0), ((32, 32), "fisheye", 180.0), ((32, 32), "fisheye", 360.0)])
@pytest.mark.parametrize("S", (1, 2, 3, 4))
def test_constant_faces_come_out_exactly_constant(case, S):
    size, projection, aperture = case
    x, y = _centres(size)
    for value in (0.0, 1.0, 0.3):
        for apron in (1, 4):
            got = ref.panorama(np.full((6, N, N, 3), value, F), size, projection, aperture, apron, S, OBLIQUE)
            if projection == "equirect":
                assert (got.view(np.uint32) == F(value).view(np.uint32)).all(), (value, apron)
                continue
            # the circle: every sub-position of a pixel inside gives the constant, every one outside 0; pixels the circle cuts lie between
            w = size[0]
            corners = [np.hypot(2.0 * (x + dx) / w - 1.0, 2.0 * (y + dy) / w - 1.0) for dx in (-0.5, 0.5) for dy in (-0.5, 0.5)]
            inner, outer = np.max(corners, 0) < 1.0, np.min(corners, 0) > 1.0
            assert inner.sum() > 600 and outer.sum() > 100
            assert (got[inner].view(np.uint32) == F(value).view(np.uint32)).all(), (value, apron)
            assert (got[outer] == 0).all()
            cut = ~inner & ~outer
            assert (got[cut] >= 0).all() and (got[cut] <= F(value)).all()


def test_the_default_sincos_is_the_device_sequence_on_exact_points():
    s, c = ref.de_sincos(np.array([0.0, np.pi / 2, np.pi, -np.pi / 2, 1e-3], F))
    assert s[0] == 0 and c[0] == 1 and abs(s[1] - 1) <= 1e-7 and abs(c[2] + 1) <= 1e-7 and abs(s[3] + 1) <= 1e-7
    x = np.linspace(-7.0, 7.0, 4001).astype(F)
    s, c = ref.de_sincos(x)
    assert np.abs(s - np.sin(x.astype(np.float64))).max() < 3e-7 and np.abs(c - np.cos(x.astype(np.float64))).max() < 3e-7
    a, b, cc = F(1.0 + 2.0 ** -23), F(1.0 - 2.0 ** -23), F(-1.0)      # a b + c = -2^-46 exactly: a plain float64 sum then float32 keeps it too
    assert ref.fma(a, b, cc) == F(-2.0 ** -46)


@pytest.mark.parametrize("sign", (1.0, -1.0))
def test_the_float64_sphere_stays_under_the_orientation_tests_cap(sign):
    """tests/test_gpu_panorama.py's orientation test on the float64 sphere alone: masks of the six face cameras' pixel centres (1 inside the planet's
    angular radius around the centre direction), resampled at S = 1; values strictly between 0 and 1 are under 10 % of the frame, every 1 lies
    inside the radius plus two face pixels' angle and every 0 outside the radius minus it."""
    size, apron = (64, 32), 1
    centre = sign * np.ones(3) / np.sqrt(3.0)
    radius = np.arcsin(1.0 / 1.5)
    idx = np.arange(N, dtype=np.float64)
    X, Y = np.meshgrid(idx, idx, indexing="ij")
    masks = np.zeros((6, N, N, 3), F)
    for f in range(6):
        look, up, fov = ref.f64_face_camera(f, N, apron)
        d = ref.f64_cast_dir(look, up, fov, N, X, Y)
        masks[f] = (np.arccos(np.clip(d @ centre, -1, 1)) < radius)[..., None]
    got = ref.panorama(masks, size, "equirect", 180.0, apron, 1)[..., 0]
    x, y = _centres(size)
    d, _ = ref.f64_direction(x, y, size, "equirect")
    ang = np.arccos(np.clip(d @ centre, -1, 1))
    margin = 2.0 * (2.0 * (N / (N - 2.0 * apron)) / N)
    between = (got > 0) & (got < 1)
    print("float64 sphere, centre %+d: %.2f %% of the frame strictly between 0 and 1" % (sign, 100.0 * between.mean()))
    assert between.mean() < 0.10
    assert (ang[got == 1] <= radius + margin).all() and (ang[got == 0] >= radius - margin).all()
    assert (got == 1).sum() > 100 and (got == 0).sum() > 1000


# ---------------------------------------------------------------- the multi-tile shapes reach what they are there for
def _ceil_div(a, b):
    return -(-a // b)


def test_the_multi_tile_shapes_reach_what_they_are_there_for():
    """tests/test_gpu_panorama.py runs ref.MULTI_TILE through the kernel; here, in numpy, what each shape is there for (panorama_kernel decodes its
    one-dimensional grid as i0 = (block / tiles_j) 32, j0 = (block % tiles_j) 32 and stages 32 S table entries per axis)."""
    T = ref.TILE
    want = {((96, 40), "equirect"): ((3, 2), (0, 8)), ((48, 72), "equirect"): ((2, 3), (16, 8)),
            ((48, 48), "fisheye"): ((2, 2), (16, 16)), ((80, 80), "fisheye"): ((3, 3), (16, 16))}
    assert len(ref.MULTI_TILE) == 4
    for size, projection, aperture in ref.MULTI_TILE:
        w, h = size
        tiles, rest = want[(size, projection)]
        assert (_ceil_div(w, T), _ceil_div(h, T)) == tiles and (w % T, h % T) == rest
        assert tiles[1] > 1                                        # more than one tile along the second axis: j0 > 0 runs
        assert w % 16 == 0 and h % 8 == 0                          # the header's size rule
        if projection == "equirect":
            assert tiles[0] != tiles[1]                            # a swapped / and % leaves a tile of the output unwritten
            assert rest[1] != 0                                    # the last tile row is partial: the in_j guard decides
        else:
            assert rest[0] != 0 and rest[1] != 0
    assert any(r[0] != 0 and r[1] != 0 for (_, p), (_, r) in want.items() if p == "equirect")      # an equirect partial on both axes
    assert T * ref.MAX_S == 128                                    # S = 4: a tile's table span is 128 entries, the LDS tables' size
    for size in ((96, 40), (48, 72)):                              # ... and the last tile of either axis reaches past the tables' end at S = 4, or ends on it
        for n in size:
            assert (_ceil_div(n, T) - 1) * T * ref.MAX_S + 128 >= n * ref.MAX_S
    assert {n for n, _ in ref.FACE_SIZES} == {16, 40} and 40 > T and 40 & 39 and 40 * 3 == 120 and all(1 <= a <= n // 4 for n, a in ref.FACE_SIZES)
    # the fisheyes: at 90° no sample leaves +f and its four neighbours; at 220° some lie behind the equator of the frame (cf < 0)
    for basis in (None, OBLIQUE):
        k = ref.consts(N, 1, 90.0, basis)
        cr, cu, cf, outside = ref.sub_direction((48, 48), "fisheye", 1, 0, 0, k)
        face, _, _ = ref.locate(cr, cu, cf, N, k)
        seen = set(np.unique(face[~outside]).tolist())
        assert 4 in seen and 5 not in seen and (face[~outside] == 4).mean() > 0.5
        k = ref.consts(N, 1, 220.0, basis)
        cr, cu, cf, outside = ref.sub_direction((80, 80), "fisheye", 1, 0, 0, k)
        face, _, _ = ref.locate(cr, cu, cf, N, k)
        assert (cf[~outside] < 0).sum() > 100 and set(np.unique(face[~outside]).tolist()) == {0, 1, 2, 3, 4}
        assert outside.any() and not outside[40, 40]


# ---------------------------------------------------------------- the resampled IMAGE against float64
LINEAR_CASES = ref.MULTI_TILE + [((32, 32), "fisheye", 360.0)]


def linear_error(got, size, projection, aperture, basis, S):
    """`got`, a panorama of ref.f64_linear_faces, against ref.f64_linear_image: the largest absolute error over the pixels all of whose sub-positions
    lie inside the image; every pixel all of whose sub-positions lie beyond the fisheye's circle must be exactly 0."""
    want, inside, outside = ref.f64_linear_image(size, projection, aperture, basis, S)
    assert got.shape == want.shape and got.dtype == F
    assert inside.sum() > inside.size // 2
    assert (got[outside] == 0).all()
    if projection == "fisheye":
        assert outside.sum() > 50
        cut = ~inside & ~outside                                   # pixels the circle cuts (none at S = 1): the mean counts a 0 per sub-position beyond it
        assert (S > 1) == bool(cut.any())
        return float(np.abs(got.astype(np.float64) - want)[~outside].max())
    assert inside.all()
    return float(np.abs(got.astype(np.float64) - want).max())


@pytest.mark.parametrize("S", (1, 4))
@pytest.mark.parametrize("case", LINEAR_CASES)
def test_linear_faces_come_out_as_the_float64_direction_field(case, S):
    """The tap addressing (u N + v) 3 + c, the choice of the four taps and the order of the two lerps, held to something that is not written from
    the header: faces whose content is linear in (u, v) (ref.f64_linear_faces, from the float64 face cameras alone) come out, at every pixel inside
    the image, as D / max |component of D| of the pixel's float64 direction D — on both sides of every cube edge, so no pixel is excluded.  A
    transposed or shifted tap is an error of fov / N = 0.07 at N = 16.  The bound: ref.LINEAR_BOUND, four times the largest error of this very
    restatement over all of these cases (measured 5.7e-7 at S = 1 where values reach 2)."""
    size, projection, aperture = case
    worst = 0.0
    for apron in (1, 4):
        for basis in (None, OBLIQUE):
            faces = ref.f64_linear_faces(N, apron, basis)
            assert 1.0 < np.abs(faces).max() <= 2.0 * np.sqrt(3.0) and len(np.unique(faces.reshape(-1, 3), axis=0)) == faces.size // 3      # no two pixels alike
            got = ref.panorama(faces, size, projection, aperture, apron, S, basis)
            err = linear_error(got, size, projection, aperture, basis, S)
            print("linear field %s S %d apron %d %s: max error %.3e" % (case, S, apron, "oblique" if basis is not None else "axes", err))
            worst = max(worst, err)
    assert worst <= ref.LINEAR_BOUND[S], (worst, ref.LINEAR_BOUND[S])      # 4 x the measured maximum of the restatement alone (ref.LINEAR_MEASURED)
    assert worst > 0.0                                             # float32 did round: the comparison is not of a thing with itself


def test_the_linear_field_catches_a_transposed_face():
    """The check's own strength: faces handed over with u and v exchanged — every tap read at (v, u), what a transposition shared by the header,
    the kernel and the restatement would be — miss the float64 field by four orders more than the bound."""
    size, projection, aperture = (96, 40), "equirect", 180.0
    faces = ref.f64_linear_faces(N, 1)
    err = linear_error(ref.panorama(np.ascontiguousarray(faces.transpose(0, 2, 1, 3)), size, projection, aperture, 1, 1), size, projection, aperture, None, 1)
    assert err > 1e4 * ref.LINEAR_BOUND[1]
