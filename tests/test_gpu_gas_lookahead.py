"""The gas stage of render_kernel_v6 reads its densities from the altitude table ONE STEP AHEAD (csrc/de_stages.h: GasStageT<true>): a trip of the
wave loop makes the collision draw of the point it holds, flies to the next point, consumes the held point's densities, issues the next point's
read and resolves the held point.  Nothing may change: every frame below is the wave-level state machine's (kernel variant 2), bit for bit
(uint32 view of the HDR frame, fraction 1.0), on the same context settings.  The cases are the ones where THIS change can go wrong: long gas
segments and ratio tracking to the sun (limb view), records suspended between `advance` and `resolve` and resumed through restore() — by yields
and by the tail's export / import —, the table's first entry, and the fixed-wavelength flag.  Small frames: 64x64 x 4 spp = 16 384 paths, four
above the threshold from which the default runs render_kernel_v6 anyway; the variant is forced.

The table's top.  The table covers altitudes below DE_DENS_TABLE_N / 2 = 131 072 m; the atmosphere's upper boundary is the compile-time constant
DE_ATMOS_UPPER = 6371 km + 110 km wherever the camera is, and a gas segment ends where the ray leaves it: the path tracer never resolves a step
above the table, so no frame can reach the stage's off-table branch (only a lane that has LEFT its segment looks ahead to such a point; it reads
a clamped entry that nothing consumes — the camera above the table below has every primary ray do that).  The read itself — clamp, truncation,
byte offset, the `h2 < DE_DENS_TABLE_N` edge, the evaluated profiles off the table — is therefore held to get_density on the index boundary as a
leaf, through de_debug_math (the entry point of tests/test_gpu_fast_math_leaves.py): test_density_read_on_the_index_boundary."""
import numpy as np
import pytest

from helpers import bits_equal_fraction, load_preset

pytestmark = pytest.mark.gpu

W = H = 64
SPP = 4
KW = dict(seed=17, texture_source="synthetic", texture_size=(1024, 512))


@pytest.fixture(scope="module")
def Renderer():
    from digital_earth_amd.renderer import Renderer as R
    return R


def _preset(r, name):
    p = load_preset(name)
    r.set_camera_pos(*p["pos"]); r.set_look_at(*p["look_at"]); r.set_up(*p["up"]); r.set_fov(p["fov"])
    r.set_aspect_scale(p["aspect_scale"]); r.set_sun_angle(p["sun_angle"]); r.set_sun_path_rot(p["sun_path_rot"])


def _frame(Renderer, variant, setup=None, tune=None, **kw):
    r = Renderer((W, H), (0, 1, 0), **dict(KW, **kw))
    if setup:
        setup(r)
    if tune:
        t = r.tuning()
        tune(t)
        r.set_tuning(t)
    r.set_kernel_variant(variant)
    r.accumulate(SPP)
    assert r.last_call_info()["variant"] == variant
    return r, r.fetch_hdr()


_reference = {}


def _state_machine(Renderer, key, setup=None, **kw):
    """the state machine's frame for a view: rendered once, shared, never written to"""
    if key not in _reference:
        f = _frame(Renderer, 2, setup, **kw)[1]
        f.setflags(write=False)
        _reference[key] = f
    return _reference[key]


VIEWS = {"default": lambda r: r.set_fov(0.4), "limb": lambda r: _preset(r, "config - sunset hurricane.txt")}


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_small_frame(Renderer, view):
    _, got = _frame(Renderer, 6, VIEWS[view])
    assert bits_equal_fraction(got, _state_machine(Renderer, view, VIEWS[view])) == 1.0
    assert got.max() > 0


def _yield_always(t):
    t.v6_yield_max = 63; t.v6_elsewhere_min = 1; t.v6_retry = 1
    for k in range(3):
        t.v6_service_lanes[k] = 1; t.v6_service_area[k] = 1


def _export(t):
    t.v6_tail_levels = 2; t.v6_tail_export[0] = 300; t.v6_tail_export[1] = 40; t.v6_tail_grid[0] = 64; t.v6_tail_grid[1] = 8
    t.v6_tail_min_paths = 0; t.v6_tail_when_alone = 1
    t.v6_yield_max = 0      # no yields of the ordinary kind: a record leaves a loop stage's lane early only through the export's own yield


def _with_stats(tune):
    def f(t):
        tune(t); t.v6_stats = 1
    return f


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_yields_resume_through_restore(Renderer, view):
    """yield_max at its largest, a service after every trip with an idle lane, a retry at once: a wave hands its records back at almost every dry
    service, and a gas record is stored between `advance` and `resolve` and resumed by restore() in whatever wave takes it.  The kernel's
    statistics (the instrumented instantiation: same arithmetic) show that yields happened and that the gas stage loaded more records than it
    does without yields — each resumption is one more load —; the shipped instantiation then renders the frame under the same settings."""
    want = _state_machine(Renderer, view, VIEWS[view])
    rs, fs = _frame(Renderer, 6, VIEWS[view], _with_stats(_yield_always))
    st = rs.v6_stats(48)
    r0, _ = _frame(Renderer, 6, VIEWS[view], _with_stats(lambda t: setattr(t, "v6_yield_max", 0)))
    st0 = r0.v6_stats(48)
    print("yields %d, records yielded %d; gas records loaded %d with yields, %d without" % (st[20], st[21], st[1], st0[1]))
    assert st[20] > 0 and st[21] > 0 and st[1] > st0[1]
    assert bits_equal_fraction(fs, want) == 1.0
    _, got = _frame(Renderer, 6, VIEWS[view], _yield_always)
    assert bits_equal_fraction(got, want) == 1.0


def test_tail_export_and_import(Renderer):
    """The frame's last paths exported to the pool and finished by two tail launches, forced on for this small frame (the settings of
    test_gpu_block_scheduler.py; set through de_set_tuning, which is what the environment variables of that test become): the records in the gas
    stage's lanes come back through the export's own yield and cross to the next launch as stored records.  Statistics word 7 counts the records
    a launch STARTS — new paths and imported ones —: more than the frame's paths means records were imported; and the gas stage loads more
    records than the frame has gas segments (a run with neither tail nor yields counts those): the surplus went through suspend() and restore()."""
    want = _state_machine(Renderer, "limb", VIEWS["limb"])
    rs, fs = _frame(Renderer, 6, VIEWS["limb"], _with_stats(_export))
    st = rs.v6_stats(48)
    r0, _ = _frame(Renderer, 6, VIEWS["limb"], _with_stats(lambda t: setattr(t, "v6_yield_max", 0)))      # no tail, no yields: every gas record is loaded once
    st0 = r0.v6_stats(48)
    print("records started %d for %d paths; yields %d; gas records loaded %d, %d without the tail" % (st[7], W * H * SPP, st[20], st[1], st0[1]))
    assert st[7] > W * H * SPP and st[20] > 0
    assert st[1] > st0[1]      # gas records were stored (the export's yield) and loaded again, through restore()
    assert bits_equal_fraction(fs, want) == 1.0
    _, got = _frame(Renderer, 6, VIEWS["limb"], _export)
    assert bits_equal_fraction(got, want) == 1.0


def _low_over_the_ground(r):
    r.set_camera_pos(0.0, 6371e3 + 3000.0, 0.0); r.set_look_at(0.0, 0.0, 0.0); r.set_up(0.0, 0.0, 1.0); r.set_fov(0.9)


def _above_the_table(r):
    r.set_camera_pos(0.0, 6371e3 + 140e3, 0.0); r.set_look_at(6371e3, 6371e3, 0.0); r.set_up(0.0, 1.0, 0.0); r.set_fov(0.7)


@pytest.mark.parametrize("name,setup,kw", [("low", _low_over_the_ground, dict(texture_source="constant", texture_size=None)), ("high", _above_the_table, {})])
def test_table_edges(Renderer, name, setup, kw):
    """low: a camera 3 km up, inside the atmosphere, looking straight down at the constant maps' sea-level surface (height 0 everywhere): the
    steps before the ground lie in the table's first entries, and a point whose |C| rounds to the planet's radius or below has its index clamped to 0.
    high: a camera at 140 km, above the table's top (131 072 m) and above the atmosphere, looking along the limb: segments start and end at the
    atmosphere's boundary (110 km, a constant: see the module's text), and every lane's last look-ahead lies outside it, often above the table."""
    _, got = _frame(Renderer, 6, setup, **kw)
    assert bits_equal_fraction(got, _state_machine(Renderer, name, setup, **kw)) == 1.0
    assert got.max() > 0


def test_fixed_wavelength(Renderer):
    """one LambdaNode for every path (the fixed-wavelength flag) and the sampled default: start() reads the node's extinctions for the first flight"""
    def fixed(r):
        r.set_fov(0.4); r.set_fixed_wavelength(550.0)
    _, got = _frame(Renderer, 6, fixed)
    assert bits_equal_fraction(got, _state_machine(Renderer, "fixed", fixed)) == 1.0
    assert got.max() > 0
    assert bits_equal_fraction(got, _state_machine(Renderer, "default", VIEWS["default"])) < 1.0      # the flag did change the frame


def test_density_read_on_the_index_boundary(Renderer):
    """pt::density_ahead (csrc/pt_leaves.h), the read GasStageT<true>::fetch issues, against get_density on the same device, bit for bit, three
    components each (de_debug_math 20-22 against 17-19).  N = DE_DENS_TABLE_N = 262 144 entries at h = i / 2 m.
    Inside its segment (live): entry trunc(2 h) for 2 h < N — h = 0 (index 0), 0.5, the altitudes around every profile's branch points, (N - 1) / 2
    (index N - 1), the float below N / 2 (2 h = N - 2^-6: still index N - 1) —; at 2 h = N and above, for +inf and for a NaN the profiles evaluated
    at h itself.  The stage's altitudes are multiples of 0.5 m, where the entry IS get_density(h); for the one h that is not, the entry is
    get_density(trunc(2 h) / 2) — the test states the index, not the table's use.
    Outside its segment (not live): the same entries below the table's top; from there on, for +inf and for a NaN the clamped entry N - 1, never an
    evaluation."""
    r = Renderer((16, 8), (0, 1, 0), texture_source="constant")
    N = 262144
    top = np.float32(N / 2)
    below_top = np.nextafter(top, np.float32(0), dtype=np.float32)
    in_table = np.array([0.0, 0.5, 1.0, 1299.5, 1300.0, 1300.5, 2400.0, 2400.5, 11500.0, 11500.5, 15000.0, 25000.0, 109999.5, (N - 1) / 2, below_top], dtype=np.float32)
    off_table = np.array([top, top + np.float32(0.5), 2.0e5, 8.0e6, np.inf, np.nan], dtype=np.float32)
    h = np.concatenate([in_table, off_table])
    index_h = (np.floor(in_table.astype(np.float64) * 2.0) / 2.0).astype(np.float32)      # the altitude of entry trunc(2 h)
    assert index_h[-1] == np.float32((N - 1) / 2) and index_h[-2] == np.float32((N - 1) / 2) and index_h[0] == 0
    want_live = np.concatenate([index_h, off_table])
    want_left = np.concatenate([index_h, np.full(off_table.shape, (N - 1) / 2, dtype=np.float32)])
    for comp in range(3):
        live = r.debug_math(20 + comp, h, np.ones_like(h)).view(np.uint32)
        left = r.debug_math(20 + comp, h, np.zeros_like(h)).view(np.uint32)
        ref_live = r.debug_math(17 + comp, want_live).view(np.uint32)
        ref_left = r.debug_math(17 + comp, want_left).view(np.uint32)
        print("component %d: live mismatches %s, left mismatches %s" % (comp, h[live != ref_live], h[left != ref_left]))
        assert (live == ref_live).all() and (left == ref_left).all()
    assert np.isfinite(r.debug_math(17, in_table)).all() and r.debug_math(17, in_table[:1])[0] > 0
