"""The panorama stage's restatement (tests/panorama_ref.py) held to an independent float64 statement of its geometry, without a GPU:
the resampler inverts the renderer's own camera, picks the face the float64 direction picks, keeps constants exactly, and the float64 sphere of the
orientation test stays under that test's cap."""
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
