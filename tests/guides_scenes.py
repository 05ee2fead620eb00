"""The maps, views and bounds shared by tests/test_guides_f64.py (CPU) and tests/test_gpu_denoise_guides.py (GPU).

Maps: 512x256, closed-form functions of longitude and latitude, no files and no RNG.  Every map carries a term linear in longitude, so that it is
discontinuous across the texture seam (u = 0 | 1, the meridian through +x): there the wrap and clamp address modes filter different texels.
  height   smooth low-frequency relief over the full byte range; the normalised relief is raised to the
           fourth power, so that with LAND_HEIGHT_SCALE = 30 km most land lies below the cloud shell (4 to 10 km) and the ranges rise tens of kilometres
  albedo   green, desert and blue regions with smooth transitions (a gradient everywhere: a wrong texture coordinate or sub-pixel offset shows)
  ocean    0, 1 and intermediate values
  clouds   0 (clear) to 1
Views: a far whole-disc view, a near oblique view over relief, a far view centred on the seam, and a close view of the seam.  The far views use aspect_scale = 20: the disc is a tall
narrow ellipse on the image.  A pixel of partial coverage holds the limb, and a hit within 3 % of the disc's radius of the limb is steeper than cos 0.2
and masked (guides_f64); only where that band is well below the half-pixel spacing of the four rays do partial pixels stay unmasked, which a round disc
large enough to have 50 limb pixels never offers.  The squeezed disc does, along its long sides, and aspect_scale gets exercised on the way."""
import numpy as np

W_MAP, H_MAP = 512, 256
LAND_HEIGHT_SCALE = 30000.0
SIZES = ((80, 40), (128, 64))
PLANET_R = 6371e3


def direction(lon_deg, lat_deg):
    """The unit vector whose sphere_UV_map is (lon / 360, lat / 180 + 0.5)."""
    a, p = np.radians(lon_deg) - np.pi, np.radians(lat_deg)
    return np.array([-np.cos(a) * np.cos(p), np.sin(p), np.sin(a) * np.cos(p)])


def _smooth(x, lo, hi):
    t = np.clip((x - lo) / (hi - lo), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t)


def make_maps():
    lon = (2.0 * np.pi * (np.arange(W_MAP) + 0.5) / W_MAP)[None, :]
    lat = (np.pi * ((np.arange(H_MAP) + 0.5) / H_MAP - 0.5))[:, None]
    ramp = lon / (2.0 * np.pi) + 0.0 * lat
    f = np.sin(3.0 * lon + 0.4) * np.cos(lat) ** 2 + 0.6 * np.sin(2.0 * lon + 1.0) * np.sin(3.0 * lat) + 0.8 * ramp
    height = np.rint(((f - f.min()) / (f.max() - f.min())) ** 4 * 255.0).astype(np.uint8)[..., None]
    s = np.sin(2.0 * lon + 0.3) * np.cos(lat) + 0.4 * np.sin(5.0 * lat)
    green, desert = _smooth(s, 0.1, 0.6)[..., None], _smooth(-s, 0.1, 0.6)[..., None]
    rgb = (1.0 - green - desert) * np.array([30.0, 60.0, 160.0]) + green * np.array([60.0, 150.0, 50.0]) + desert * np.array([215.0, 180.0, 120.0])
    albedo = np.rint(rgb * (0.7 + 0.3 * ramp[..., None])).astype(np.uint8)
    ocean = np.rint(255.0 * np.clip(0.5 + 1.5 * np.sin(2.0 * lon + 2.0) * np.cos(2.0 * lat) + 0.3 * (ramp - 0.5), 0.0, 1.0)).astype(np.uint8)[..., None]
    clouds = np.rint(255.0 * np.clip(0.5 + 0.9 * np.sin(4.0 * lon) * np.sin(3.0 * lat + 0.5) + 0.4 * (ramp - 0.5), 0.0, 1.0)).astype(np.uint8)[..., None]
    return dict(height=height, albedo=albedo, ocean=ocean, clouds=clouds)


def _cam(pos, look_at, fov, aspect_scale=1.0):
    # through float32: what the renderer holds
    f = lambda x: [float(np.float32(c)) for c in x]
    return dict(pos=f(pos), look_at=f(look_at), up=[0.0, 1.0, 0.0], fov=float(np.float32(fov)), aspect_scale=float(aspect_scale), land_height_scale=LAND_HEIGHT_SCALE, topo_res=0)


VIEWS = {
    "far": _cam(1.04e7 * direction(230.0, 20.0), (0.0, 0.0, 0.0), 0.85, 20.0),
    "near": _cam(7.2e6 * direction(200.0, 10.0), PLANET_R * direction(203.0, 12.0), 0.3),
    "seam": _cam(1.0e7 * direction(0.0, 12.0), (0.0, 0.0, 0.0), 0.85, 20.0),
    # straight down on the seam from 830 km: about 1000 km across, of which the texel column that the two address modes filter differently (78 km, and
    # the land_normal taps 39 km to either side) is a tenth.  A view whose hits span u < 0.05 to u > 0.95 cannot show that column on more than 2 % of its width.
    "seam_close": _cam(7.2e6 * direction(0.0, 12.0), (0.0, 0.0, 0.0), 0.3),
}
FAR_VIEWS = ("far", "seam")

# The measured basis: the largest deviation, over every view, size and address mode, of the guides composed in float32 from the oracle's probes from the
# float64 guides on unmasked pixels (tests/test_guides_f64.py measures and asserts them).  distance: relative; normal: 1 - dot; albedo, transmittance: absolute.
# Measured: distance 2.864e-6 (far 80x40), normal 1.451e-7 (seam 80x40), albedo 5.253e-6 (seam 80x40), transmittance 5.833e-5 (seam 128x64): the constants
# are these figures rounded up in the third digit, no more.
BASIS = dict(distance=2.87e-6, normal=1.46e-7, albedo=5.26e-6, transmittance=5.84e-5)
# The constant-map test's bounds (tests/test_gpu_denoise.py): the GPU bounds are four times the basis and never looser than these.
EXISTING = dict(distance=1e-3, normal=1.0 - 0.9999, albedo=1e-5, transmittance=2e-3)


def bounds():
    return {k: min(4.0 * BASIS[k], EXISTING[k]) for k in BASIS}


def deviations(got, want):
    """Per pixel: (coverage differs, distance relative, 1 - normal dot, albedo max abs, transmittance abs) of guides (W, H, 9) against the reference's."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    land = want[..., 0] > 0
    dist = np.where(land, np.abs(got[..., 1] - want[..., 1]) / np.maximum(want[..., 1], 1.0), np.abs(got[..., 1]))
    nrm = np.where(land, 1.0 - (got[..., 2:5] * want[..., 2:5]).sum(-1), np.abs(got[..., 2:5]).max(-1))
    return dict(coverage=got[..., 0] != want[..., 0], distance=dist, normal=nrm, albedo=np.abs(got[..., 5:8] - want[..., 5:8]).max(-1),
                transmittance=np.abs(got[..., 8] - want[..., 8]))
