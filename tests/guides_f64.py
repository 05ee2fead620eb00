"""A float64 numpy statement of the denoiser's guides, written from the reference's definitions as the oracle restates them
(oracle/oracle_lib.h: sphere_UV_map, sample_lod, sample_sphere_texture; oracle/oracle_pathtracer.h: land_sdf, land_normal, intersect_land,
get_clouds_density, get_land_material) and from the guides' definition: four rays per pixel at the sub-pixel offsets (0.25 | 0.75, 0.25 | 0.75),
coverage = hits / 4, distance = mean over the hitting rays, normal = the normalised sum, albedo = sum / 4, transmittance = the mean of
exp(-0.1 sum(density) dt) over 64 midpoint steps through the upper cloud sphere.  It shares no code with the kernel.  Vectorised over rays.

Maps are uint8 arrays [height][width][channels], row 0 = south.  Positions and directions are (N, 3) float64.

THE AMBIGUITY MASK.  The kernel works in float32, this statement in float64, and the guides hold decisions: a ray hits or misses, the sphere trace
stops at this step or the next, a cloud sample lies inside the shell or outside.  Where float32 rounding can flip one, the two legitimately differ
by far more than rounding, so guides() also returns a per-pixel mask, true where a decision of any of the pixel's four rays is that close:
  * the sphere trace's stop test |d| < 1e-4 t with |d| within 1 % of 1e-4 t, or its maximum-distance test within 1 % of the limit (looked at after
    every step, the last two included: a step that nearly stopped earlier is the same decision);
  * hit or miss: a missing ray whose closest approach to the terrain (the smallest signed distance its trace saw) is below 5 km, and a ray whose
    250 steps ran out before either test decided;
  * a hit at an incidence steeper than cos 0.2 (the trace stops within 1e-4 t of the surface along the normal, 1e-4 t / cos along the ray);
  * a cloud sample within 2 m of either shell radius;
  * a cloud sample with either column-height inequality within 2e-4 of equality.
The margins follow from float32's half-metre spacing at 6.4e6 m: a radius is known to about a metre, which is 1.7e-4 of the 6 km shell (the 2e-4
and the 2 m), and a metre against the 1e-4 t stop band (hundreds of metres at these distances) is far inside 1 %."""
import numpy as np

import leaf_f64

PLANET_R = 6371e3
ATMOS_UPPER = 6371e3 + 110e3
CLOUDS_LOWER = 6371e3 + 4000.0
CLOUDS_UPPER = 6371e3 + 4000.0 + 6000.0
CLOUDS_THICKNESS = 6000.0
CLOUDS_DENSITY = 0.029
CLOUDS_EXTINCT = 0.1
MAX_RAY_DIST = 6371e3 * 10.0
SPHERE_STEPS = 250
CLOUD_STEPS = 64
OFFSETS = ((0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75))

STOP_BAND = 0.01          # relative distance of |d| from 1e-4 t, and of t from the maximum distance
MISS_MARGIN = 5e3         # m
STEEP_COS = 0.2
SHELL_MARGIN = 2.0        # m
COLUMN_MARGIN = 2e-4


# ---------------------------------------------------------------- textures
def sphere_UV_map(n):
    """Unit vectors (..., 3) -> (u, v): u = (atan2(z, -x) / pi + 1) / 2, v = asin(y) / pi + 0.5."""
    n = np.asarray(n, np.float64)
    return (np.arctan2(n[..., 2], -n[..., 0]) / np.pi + 1.0) / 2.0, np.arcsin(np.clip(n[..., 1], -1.0, 1.0)) / np.pi + 0.5


def sample_lod(tex, u, v, clamp):
    """Bilinear fetch at normalised (u, v), texel centres at (i + 0.5) / N, address mode wrap (repeat) or clamp; bytes scale by 1 / 255.  (..., channels)."""
    t = np.asarray(tex, np.float64)
    h, w = t.shape[:2]
    x, y = np.asarray(u, np.float64) * w - 0.5, np.asarray(v, np.float64) * h - 0.5
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[..., None], (y - y0)[..., None]

    def addr(i, n):
        return np.clip(i, 0, n - 1) if clamp else np.mod(i, n)
    i0, i1 = addr(x0.astype(np.int64), w), addr(x0.astype(np.int64) + 1, w)
    j0, j1 = addr(y0.astype(np.int64), h), addr(y0.astype(np.int64) + 1, h)
    a = t[j0, i0] * (1.0 - fx) + t[j0, i1] * fx
    b = t[j1, i0] * (1.0 - fx) + t[j1, i1] * fx
    return (a * (1.0 - fy) + b * fy) / 255.0


def sample_sphere_texture(tex, pos, clamp):
    pos = np.asarray(pos, np.float64)
    u, v = sphere_UV_map(pos / np.linalg.norm(pos, axis=-1, keepdims=True))
    return sample_lod(tex, u - np.floor(u), v - np.floor(v), clamp)


# ---------------------------------------------------------------- terrain
def land_sdf(height, pos, scale, clamp):
    return np.linalg.norm(pos, axis=-1) - PLANET_R - scale * sample_sphere_texture(height, pos, clamp)[..., 0]


def land_normal(height, topo_res, pos, scale, clamp):
    e = np.pi * 6371e3 / topo_res
    d = land_sdf(height, pos, scale, clamp)
    n = np.stack([d - land_sdf(height, pos - np.array(o) * e, scale, clamp) for o in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))], -1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def _sphere(pos, dirs, radius):
    """Entry and exit distances of the sphere |p| = radius along the rays, and the discriminant (negative: no intersection)."""
    b = dirs @ pos
    disc = b * b - pos @ pos + radius * radius
    s = np.sqrt(np.maximum(disc, 0.0))
    return -b - s, -b + s, disc


def intersect_land(height, pos, dirs, scale, clamp):
    """The sphere trace: up to 250 steps from the atmosphere entry (from the origin if that lies behind or is missed), stopping when the travelled
    distance passes the maximum or |d| < 1e-4 t.  Returns (t, or -1 for a miss; steps taken; a dict of per-ray decision margins)."""
    pos, dirs = np.asarray(pos, np.float64), np.asarray(dirs, np.float64)
    n = dirs.shape[0]
    t_in, _, disc = _sphere(pos, dirs, ATMOS_UPPER)
    t = np.where((disc >= 0.0) & (t_in > 0.0), t_in, 0.0)
    steps = np.zeros(n, np.int64)
    near_band = np.zeros(n, bool)
    min_sdf = np.full(n, np.inf)
    active = np.arange(n)
    for _ in range(SPHERE_STEPS):
        if active.size == 0:
            break
        d = land_sdf(height, pos + dirs[active] * t[active, None], scale, clamp)
        t[active] += d
        ta = t[active]
        steps[active] += 1
        min_sdf[active] = np.minimum(min_sdf[active], d)
        near_band[active] |= (np.abs(np.abs(d) - 1e-4 * ta) <= STOP_BAND * 1e-4 * np.abs(ta)) | (np.abs(ta - MAX_RAY_DIST) <= STOP_BAND * MAX_RAY_DIST)
        active = active[~((ta > MAX_RAY_DIST) | (np.abs(d) < ta * 1e-4))]
    exhausted = np.zeros(n, bool)
    exhausted[active] = True
    hit = t < MAX_RAY_DIST
    return np.where(hit, t, -1.0), steps, dict(near_band=near_band, exhausted=exhausted, grazing_miss=~hit & (min_sdf < MISS_MARGIN), min_sdf=min_sdf)


def get_land_material(albedo, ocean, pos, clamp):
    """(albedo_srgb (N, 3), ocean (N,)): the colour grade of the albedo texel towards the ocean albedo by the ocean mask."""
    o = sample_sphere_texture(ocean, pos, clamp)[..., 0]
    return leaf_f64.grade_land_albedo(sample_sphere_texture(albedo, pos, clamp), o), o


# ---------------------------------------------------------------- clouds
def get_clouds_density(clouds, pos, clamp, margins=False):
    """Density at the points; with margins also a mask of the points where a float32 radius could decide the shell or column-height tests otherwise."""
    r = np.linalg.norm(pos, axis=-1)
    inside = (r > CLOUDS_LOWER) & (r < CLOUDS_UPPER)
    h = (r - CLOUDS_LOWER) / CLOUDS_THICKNESS
    c = sample_sphere_texture(clouds, pos, clamp)[..., 0]
    split = 0.2
    column = (h - split < c * (1.0 - 0.2)) & (split - h < c * split)
    density = np.where(inside & column, np.maximum(c, 0.4), 0.0) * CLOUDS_DENSITY
    if not margins:
        return density
    shell = np.minimum(np.abs(r - CLOUDS_LOWER), np.abs(r - CLOUDS_UPPER)) < SHELL_MARGIN
    edge = inside & ((np.abs(h - split - c * 0.8) < COLUMN_MARGIN) | (np.abs(split - h - c * split) < COLUMN_MARGIN))
    return density, shell | edge


def cloud_samples(pos, dirs, t_land):
    """The 64 midpoints (N, 64, 3) and the step dt (N,; 0 where the ray has no segment): from max(t_in, 0) to min(t_out, t_land) of the upper cloud sphere."""
    t_in, t_out, disc = _sphere(pos, dirs, CLOUDS_UPPER)
    t0 = np.maximum(t_in, 0.0)
    t1 = np.where(t_land > 0.0, np.minimum(t_out, t_land), t_out)
    ok = (disc >= 0.0) & (t1 > t0)
    dt = np.where(ok, (t1 - t0) / CLOUD_STEPS, 0.0)
    ts = t0[:, None] + (np.arange(CLOUD_STEPS) + 0.5)[None, :] * dt[:, None]
    return pos + dirs[:, None, :] * ts[..., None], dt


# ---------------------------------------------------------------- camera
def camera_basis(cam):
    d = np.asarray(cam["look_at"], np.float64) - np.asarray(cam["pos"], np.float64)
    d /= np.linalg.norm(d)
    du = np.cross(d, np.asarray(cam["up"], np.float64)); du /= np.linalg.norm(du)
    dv = np.cross(du, d); dv /= np.linalg.norm(dv)
    return d, du, dv


def ray_dirs(cam, W, H, ou, ov):
    """Unit directions (W, H, 3) through (pixel + (ou, ov))."""
    d, du, dv = camera_basis(cam)
    fov, asp, scale = float(cam["fov"]), W / H, float(cam.get("aspect_scale", 1.0))
    u = np.arange(W)[:, None] + ou
    v = np.arange(H)[None, :] + ov
    fu = (2 * fov * u / H - fov * asp - 1e-5) * scale
    fv = 2 * fov * v / H - fov - 1e-5 + 0 * u
    dirs = d + fu[..., None] * du + fv[..., None] * dv
    return dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)


# ---------------------------------------------------------------- the guides
def trace(maps, cam, dirs, clamp):
    """Everything one ray contributes, for rays (N, 3) from the camera: hit, t, steps, normal, albedo, u of the hit, transmittance, and `ambiguous`."""
    pos = np.asarray(cam["pos"], np.float64)
    scale = float(cam["land_height_scale"])
    topo_res = cam.get("topo_res") or np.asarray(maps["height"]).shape[1]
    t, steps, m = intersect_land(maps["height"], pos, dirs, scale, clamp)
    hit = t > 0.0
    hp = pos + dirs[hit] * t[hit, None]
    n = dirs.shape[0]
    normal, albedo, hit_u = np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, np.nan)
    normal[hit] = land_normal(maps["height"], topo_res, hp, scale, clamp)
    albedo[hit] = get_land_material(maps["albedo"], maps["ocean"], hp, clamp)[0]
    hit_u[hit] = sphere_UV_map(hp / np.linalg.norm(hp, axis=-1, keepdims=True))[0]
    steep = hit & (np.abs((dirs * normal).sum(-1)) < STEEP_COS)
    pts, dt = cloud_samples(pos, dirs, t)
    dens, edge = get_clouds_density(maps["clouds"], pts.reshape(-1, 3), clamp, margins=True)
    dens, edge = dens.reshape(n, CLOUD_STEPS), edge.reshape(n, CLOUD_STEPS) & (dt > 0.0)[:, None]
    trans = np.exp(-CLOUDS_EXTINCT * dens.sum(-1) * dt)
    ambiguous = m["near_band"] | m["exhausted"] | m["grazing_miss"] | steep | edge.any(-1)
    return dict(hit=hit, t=t, steps=steps, normal=normal, albedo=albedo, hit_u=hit_u, trans=trans, ambiguous=ambiguous, cloud_points=pts, cloud_dt=dt,
                cloud_density=dens, why=dict(m, steep=steep, cloud_edge=edge.any(-1)))


def guides(maps, cam, W, H, clamp, offsets=OFFSETS):
    """(guides (W, H, 9) = coverage, distance, normal xyz, albedo rgb, transmittance; the ambiguity mask (W, H); the four rays' traces)."""
    rays = []
    for ou, ov in offsets:
        rays.append(trace(maps, cam, ray_dirs(cam, W, H, ou, ov).reshape(-1, 3), clamp))
    hits = np.sum([r["hit"] for r in rays], 0).astype(np.float64)
    g = np.zeros((W * H, 9))
    g[:, 0] = hits / 4.0
    g[:, 1] = np.sum([np.where(r["hit"], r["t"], 0.0) for r in rays], 0) / np.maximum(hits, 1.0)
    nsum = np.sum([r["normal"] for r in rays], 0)
    ln = np.linalg.norm(nsum, axis=-1, keepdims=True)
    g[:, 2:5] = np.where(ln > 0.0, nsum / np.maximum(ln, 1e-300), 0.0)
    g[:, 5:8] = np.sum([r["albedo"] for r in rays], 0) / 4.0
    g[:, 8] = np.sum([r["trans"] for r in rays], 0) / 4.0
    mask = np.any([r["ambiguous"] for r in rays], 0)
    return g.reshape(W, H, 9), mask.reshape(W, H), rays
