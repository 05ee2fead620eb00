"""The seeded parameter sweep of the path tracer: 48 valid configurations that combine what the hand-picked scenes of the suite vary one at a time.

`cases()` is a pure function: a constant seed, no clock, no environment, no oracle and no GPU.  The list is stratified, not blindly random: every
axis below has named strata, and case i takes, on each axis, slot (i * stride + offset) mod 48 of that axis's table of 48 stratum names — a
permutation of the cases per axis, the strides all co-prime to 48 and different from axis to axis (the two-level cycling of
tests/test_gpu_exr_aovs.py's CASES, with 16 axes instead of four).  The tables are weighted where a stratum is dark by construction — 830 nm has no CIE response, a
deep-night view and a narrow view of space show nothing — and the strides and offsets were searched once so that those strata coincide (at most 6
black frames: tests/test_sweep_cases.py counts them on the oracle) and that the strata of different axes meet as widely as 48 cases allow.  The
continuous values inside a stratum come from numpy.random.default_rng((SEED, i)).

tests/test_sweep_cases.py renders every case on the CPU oracle alone and checks what the sweep reaches; tests/test_gpu_parameter_sweep.py holds
the kernels to the oracle on it, bit for bit.  `apply(case, params)` writes a case into a de_params structure (the product's or the oracle's: same
layout) so that both files render the same bits of input."""
import math

import numpy as np

SEED = 20261021
N_CASES = 48
R = 6371e3                                  # planet radius, metres
SHELL = (R + 4000.0, R + 10000.0)           # the cloud shell (DE_CLOUDS_LOWER, DE_CLOUDS_UPPER)
ATMOSPHERE = R + 110e3                      # DE_ATMOS_UPPER
FRAME = (64, 32)
SPP = 2
DEFAULT_SCALE = 7800.0                      # de_params.land_height_scale as de_create leaves it
# The wavelength table: 441 entries, one per nanometre from 390 nm (luts.CIE_LUT_RES, luts.O3_CROSSEC_LUT_RES; LambdaNode's wavelength = 390 + 441 mid
# in csrc/aux_kernels.hip).  Its first and last nodes:
LAMBDA_FIRST, LAMBDA_LAST = 390.0, 830.0

FLAG_FIXED_WAVELENGTH, FLAG_CLAMP_SAMPLER, FLAG_RAY_MARCHER = 1 << 0, 1 << 1, 1 << 2      # include/digital_earth.h: DE_FLAG_*

# map sizes per slot (albedo, topography, ocean, clouds, bathymetry, emissive, stars): one common size, and the ragged quality-1 set of
# test_mixed_map_sizes_and_partial_tiles at a quarter of its size (203 % 8 = 3, 101 % 4 = 1, 270 % 8 = 6, 135 % 4 = 3: partial 8x4 footprint tiles
# on every map; the cloud map of another size than the topography; an odd emissive map)
MAP_SIZES = {
    "common": [(512, 256)] * 7,
    "ragged": [(270, 135), (270, 135), (203, 101), (203, 101), (270, 135), (271, 135), (203, 101)],
}
MAP_SEEDS = (20240127, 77)


def _table(*strata):
    """48 slots from (name, count) pairs, in blocks."""
    out = [name for name, count in strata for _ in range(count)]
    assert len(out) == N_CASES, len(out)
    return out


# axis -> (stride, offset, table).  Strides: the 16 units modulo 48.
AXES = {
    "height": (37, 4, _table(("below_shell", 8), ("in_shell", 8), ("10_100km", 8), ("400km", 8), ("default_distance", 8), ("10R", 8))),
    "direction": (19, 41, _table(("generic", 18), ("pole_north", 6), ("pole_south", 6), ("seam", 9), ("axis", 9))),
    "view": (11, 25, _table(("nadir", 9), ("limb", 9), ("away", 5), ("to_sun", 7), ("generic", 9), ("up_varied", 9))),
    "sun": (17, 46, _table(("day", 22), ("terminator", 20), ("night", 6))),
    "sun_path_rot": (43, 13, _table(("zero", 16), ("positive", 16), ("negative", 16))),
    "fov": (35, 39, _table(("0.02", 10), ("0.42", 20), ("1.5", 18))),
    "aspect_scale": (1, 46, _table(("0.5", 16), ("1.0", 16), ("1.25", 16))),
    "land_height_scale": (25, 41, _table(("zero", 12), ("default", 12), ("negative", 12), ("30000", 12))),
    "topo_res_override": (13, 6, _table(("0", 24), ("21600", 24))),
    "wavelength": (7, 45, _table(("spectral", 24), ("550", 12), ("first_node", 9), ("last_node", 3))),
    "sampler": (47, 31, _table(("repeat", 24), ("clamp", 24))),
    "integrator": (23, 27, _table(("path_tracer", 40), ("ray_marcher", 8))),
    "map_variant": (31, 20, _table(("default", 24), ("cloud_heavy", 24))),
    "map_sizes": (5, 9, _table(("common", 24), ("ragged", 24))),
    "map_seed": (29, 22, _table(("seed0", 24), ("seed1", 24))),
    "launch": (41, 20, _table(("one_call_of_2", 24), ("two_calls_of_1", 24))),
}


def strata_of(i):
    return {axis: table[(i * stride + offset) % N_CASES] for axis, (stride, offset, table) in AXES.items()}


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def light_direction(sun_angle, sun_path_rot):
    """Towards the sun (renderer.py:301-302, csrc/aux_kernels.hip: fc.light_dir)."""
    sa, ca = math.sin(sun_angle), math.cos(sun_angle)
    sr, cr = math.sin(sun_path_rot), math.cos(sun_path_rot)
    return np.array([-sa, ca * -sr, ca * cr])


def viewed_point(pos, d):
    """Unit direction, from the centre, of the ground the view centres on: where the central ray meets the sphere of radius R, else the point of the
    ray closest to the centre (the tangent point of a limb view), else — looking away — the point under the camera."""
    pos, d = np.asarray(pos, np.float64), _unit(d)
    b = float(np.dot(pos, d))
    if b >= 0.0:
        return _unit(pos)
    disc = b * b - (float(np.dot(pos, pos)) - R * R)
    t = -b - math.sqrt(disc) if disc > 0.0 else -b
    return _unit(pos + t * d)


def _sun_angle(n, rot, where):
    """The sun's path at `rot` is a great circle; the angle on it that puts the sun highest over n (day), lowest (night), or on n's horizon."""
    e1, e2 = np.array([1.0, 0.0, 0.0]), np.array([0.0, -math.sin(rot), math.cos(rot)])
    phi = math.atan2(float(np.dot(n, e1)), float(np.dot(n, e2)))      # n . light = A cos(angle + phi)
    return -phi + {"day": 0.0, "terminator": 0.5 * math.pi, "night": math.pi}[where]


def _f32(x):
    return float(np.float32(x))


def _case(i):
    s = strata_of(i)
    rng = np.random.default_rng((SEED, i))
    # ---- where the camera is
    kind = s["direction"]
    if kind == "generic":
        u = _unit(rng.standard_normal(3))
    elif kind in ("pole_north", "pole_south"):
        u = np.array([0.0, 1.0 if kind == "pole_north" else -1.0, 0.0])
    elif kind == "seam":      # sphere_UV_map (csrc/de_device.h): u = atan2(z, -x) / 2 pi + 1/2 wraps where z = 0 and x > 0
        lat = float(rng.uniform(0.2, 1.2)) * (1.0 if rng.integers(2) else -1.0)
        u = np.array([math.cos(lat), math.sin(lat), 0.0])
    else:
        u = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]][int(rng.integers(4))])
    h = {"below_shell": lambda: float(rng.uniform(50.0, 3900.0)),
         "in_shell": lambda: float(rng.uniform(SHELL[0] - R + 100.0, SHELL[1] - R - 100.0)),
         "10_100km": lambda: float(10.0 ** rng.uniform(4.0, 5.0)),
         "400km": lambda: 400e3,
         "default_distance": lambda: 15e6 * math.sqrt(2.0) - R,
         "10R": lambda: 9.0 * R}[s["height"]]()
    pos = np.array([_f32(x) for x in u * (R + h)])
    dist = float(np.linalg.norm(pos))
    tangent = _unit(np.cross(u, _unit(rng.standard_normal(3))))
    # ---- the sun's path; its angle follows once the view is known
    rot = {"zero": 0.0, "positive": float(rng.uniform(0.2, 1.2)), "negative": -float(rng.uniform(0.2, 1.2))}[s["sun_path_rot"]]
    # ---- where it looks
    up = np.array([0.0, 1.0, 0.0])
    view = s["view"]
    sun_angle = None
    if view == "nadir":
        d = -u
    elif view == "limb":      # tangent to a sphere 0 ... 60 km above the ground; a camera below that looks along its own horizon
        r_limb = R + float(rng.uniform(0.0, 60e3))
        alpha = math.asin(min(1.0, r_limb / dist))
        d = -u * math.cos(alpha) + tangent * math.sin(alpha)
    elif view == "away":
        d = _unit(u + 0.3 * tangent)
    elif view == "to_sun":
        sun_angle = _sun_angle(u, rot, s["sun"])
        d = light_direction(sun_angle, rot)
    else:
        d = _unit(rng.standard_normal(3) * (0.6 * R) - pos)
        if view == "up_varied":
            up = _unit(rng.standard_normal(3))
    while abs(float(np.dot(_unit(d), up))) > 0.95:      # the camera's basis needs cross(d, up) != 0: a view along `up` takes another
        up = _unit(rng.standard_normal(3)) if view == "up_varied" else np.array([0.0, 0.0, 1.0] if up[1] else [1.0, 0.0, 0.0])
    look = np.array([_f32(x) for x in pos + _unit(d) * dist])
    if view == "nadir":
        look = np.zeros(3)
    if sun_angle is None:
        sun_angle = _sun_angle(viewed_point(pos, look - pos), rot, s["sun"])
    sun_angle = math.fmod(sun_angle, 2.0 * math.pi)
    wavelength = {"spectral": None, "550": 550.0, "first_node": LAMBDA_FIRST, "last_node": LAMBDA_LAST}[s["wavelength"]]
    case = dict(
        index=i,
        pos=[float(x) for x in pos], look=[float(x) for x in look], up=[float(x) for x in up],
        fov=float(s["fov"]), aspect_scale=float(s["aspect_scale"]),
        sun_angle=_f32(sun_angle), sun_path_rot=_f32(rot),
        land_height_scale={"zero": 0.0, "default": DEFAULT_SCALE, "negative": -8000.0, "30000": 30000.0}[s["land_height_scale"]],
        topo_res_override=int(s["topo_res_override"]),
        fixed_wavelength=wavelength,
        clamp=s["sampler"] == "clamp",
        marcher=s["integrator"] == "ray_marcher",
        cloud_heavy=s["map_variant"] == "cloud_heavy",
        map_sizes=s["map_sizes"],
        map_seed=MAP_SEEDS[0 if s["map_seed"] == "seed0" else 1],
        seed=int(rng.integers(0, 1 << 20)),
        calls=[2] if s["launch"] == "one_call_of_2" else [1, 1],
        strata=s,
    )
    case["id"] = "%02d-%s-%s-%s-%s%s%s" % (i, s["height"], s["direction"], s["view"], s["sun"], "-clamp" if case["clamp"] else "",
                                         "-march" if case["marcher"] else "")
    return case


def cases():
    return [_case(i) for i in range(N_CASES)]


def map_key(case):
    """Cases with the same key render the same maps."""
    return (case["map_sizes"], case["map_seed"], case["cloud_heavy"])


def sun_cosine(case):
    """Cosine of the sun's zenith angle at the ground the view centres on."""
    pos, look = np.array(case["pos"]), np.array(case["look"])
    n = _unit(pos) if case["strata"]["view"] == "to_sun" else viewed_point(pos, look - pos)
    return float(np.dot(n, light_direction(case["sun_angle"], case["sun_path_rot"])))


def apply(case, p):
    """Write the case into a de_params structure (the product's _native.DeParams or the oracle's: one layout); what the case does not set is left."""
    up = np.array(case["up"], dtype=np.float32)
    up = (np.float32(1.0) / np.sqrt((up[0] * up[0] + up[1] * up[1]) + up[2] * up[2])) * up      # Renderer.set_up's normalisation, in f32
    for k in range(3):
        p.camera_pos[k], p.look_at[k], p.up[k] = case["pos"][k], case["look"][k], float(up[k])
    p.fov, p.aspect_scale = case["fov"], case["aspect_scale"]
    p.sun_angle, p.sun_path_rot = case["sun_angle"], case["sun_path_rot"]
    p.land_height_scale = case["land_height_scale"]
    p.topo_res_override = case["topo_res_override"]
    flags = p.flags & ~(FLAG_FIXED_WAVELENGTH | FLAG_CLAMP_SAMPLER | FLAG_RAY_MARCHER)
    if case["fixed_wavelength"] is not None:
        flags |= FLAG_FIXED_WAVELENGTH
        p.fixed_wavelength = case["fixed_wavelength"]
    if case["clamp"]:
        flags |= FLAG_CLAMP_SAMPLER
    if case["marcher"]:
        flags |= FLAG_RAY_MARCHER
    p.flags = flags
    return p
