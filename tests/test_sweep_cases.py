"""The parameter sweep of tests/sweep_cases.py, checked on the CPU oracle alone: what tests/test_gpu_parameter_sweep.py compares the kernels with is
deterministic, terminates, is finite, is not black, and reaches the events a hand-picked scene rarely does — paths to the vertex limit, deep
paths, rays that see the stars alone, cameras inside the atmosphere and inside the cloud shell — and the switches it sets change the frame.  Maps
come from Oracle.generate_texture, which test_synthetic_maps_match_cpu_statement proves byte-equal to the GPU generator.  `pytest -s` prints the
coverage table of DESIGN.md §2."""
import copy

import numpy as np
import pytest

import sweep_cases as sc

VERTEX_LIMIT = 25      # pathtracer.py:316 `for scatter_count in range(25)`; the ray marcher has no vertices beyond its first
# The vertex count of a sample counts the passes of that loop, the pass that finds nothing included: a primary ray that meets neither ground nor medium —
# space, the stars term alone — ends with a count of 1.  That is the sweep's "no vertex".
NO_VERTEX = 1
W, H = sc.FRAME


def make_oracle(case, lut_arrays):
    from oracle import oracle_binding as ob
    o = ob.Oracle(W, H)
    cie, s2s, o3, crf, _ = lut_arrays
    o.upload_luts(cie, s2s, o3, crf)
    for slot, (w, h) in enumerate(sc.MAP_SIZES[case["map_sizes"]]):
        o.generate_texture(slot, w, h, case["map_seed"], 1 if case["cloud_heavy"] else 0)
    o.set_params(sc.apply(case, o.get_params()))
    return o


def render(case, lut_arrays):
    """The oracle's frame of a case as the case launches it, with the traces of its two samples and its work counters."""
    o = make_oracle(case, lut_arrays)
    for n in case["calls"]:
        o.accumulate(n, case["seed"])
    return dict(hdr=o.fetch_hdr(), counters=o.counters(), trace=[o.debug_samples(case["seed"], k) for k in range(sc.SPP)])


@pytest.fixture(scope="module")
def rendered(lut_arrays):
    return [(c, render(c, lut_arrays)) for c in sc.cases()]


def test_cases_are_a_fixed_stratified_list():
    a, b = sc.cases(), sc.cases()
    assert a == b and len(a) == sc.N_CASES
    assert len({c["id"] for c in a}) == sc.N_CASES
    for axis, (stride, offset, table) in sc.AXES.items():
        assert np.gcd(stride, sc.N_CASES) == 1
        for stratum in set(table):
            assert sum(c["strata"][axis] == stratum for c in a) >= 3, (axis, stratum)
    assert len({stride for stride, _, _ in sc.AXES.values()}) == len(sc.AXES)


def test_cases_are_what_their_strata_say():
    for c in sc.cases():
        s, pos, look, up = c["strata"], np.array(c["pos"]), np.array(c["look"]), np.array(c["up"])
        assert np.isfinite(pos).all() and np.isfinite(look).all() and np.linalg.norm(look - pos) > 1.0      # the stated contract
        r = np.linalg.norm(pos)
        lo, hi = {"below_shell": (sc.R + 50.0, sc.R + 3900.0), "in_shell": sc.SHELL, "10_100km": (sc.R + 1e4, sc.R + 1e5), "400km": (sc.R + 399e3, sc.R + 401e3),
                  "default_distance": (2.1e7, 2.13e7), "10R": (9.99 * sc.R, 10.01 * sc.R)}[s["height"]]
        assert lo - 1.0 <= r <= hi + 1.0, c["id"]
        if s["direction"] in ("pole_north", "pole_south"):
            assert pos[0] == 0.0 and pos[2] == 0.0 and (pos[1] > 0) == (s["direction"] == "pole_north")
        if s["direction"] == "seam":
            assert pos[2] == 0.0 and pos[0] > 0.0 and pos[1] != 0.0
        if s["direction"] == "axis":
            assert np.count_nonzero(pos) == 1 and pos[1] == 0.0
        assert abs(np.linalg.norm(up) - 1.0) < 1e-6                                       # kept normalised ...
        d = (look - pos) / np.linalg.norm(look - pos)
        assert abs(np.dot(d, up)) <= 0.95 + 1e-6                                          # ... and a basis with the view
        assert (s["sun_path_rot"] == "zero") == (c["sun_path_rot"] == 0.0) and (s["sun_path_rot"] == "negative") == (c["sun_path_rot"] < 0.0)
    # the sun strata: where the sun's path passes over the viewed ground at all, the sun stands where the stratum says
    cos = {k: [sc.sun_cosine(c) for c in sc.cases() if c["strata"]["sun"] == k] for k in ("day", "terminator", "night")}
    assert sum(x > 0.5 for x in cos["day"]) >= 3 and min(cos["day"]) > -1e-6
    assert sum(x < -0.5 for x in cos["night"]) >= 3 and max(cos["night"]) < 1e-6
    assert max(abs(x) for x in cos["terminator"]) < 1e-3


def test_every_case_is_finite_and_few_are_black(rendered):
    black = [c["id"] for c, out in rendered if not out["hdr"].any()]
    for c, out in rendered:
        assert np.isfinite(out["hdr"]).all(), c["id"]
        for t in out["trace"]:
            assert np.isfinite(t).all(), c["id"]
    assert len(black) <= 6, black


def test_the_sweep_reaches_the_rare_events(rendered):
    print("\n%-52s %5s %6s %7s %9s" % ("case", "lit", "verts", "draws", "steps"))
    deep = stars = at_limit = 0
    for c, out in rendered:
        k, n = out["counters"], W * H * sc.SPP
        assert k["samples"] == n
        verts = np.stack([t[..., 3] for t in out["trace"]])
        assert verts.sum() == k["vertices"]      # the two traced samples ARE the frame's samples
        lit = int((out["hdr"] != 0).any(axis=2).sum())
        print("%-52s %5d %6.2f %7.1f %9d" % (c["id"], lit, k["vertices"] / n, k["rng_draws"] / n, k["tracking_steps"]))
        at_limit += int((verts >= VERTEX_LIMIT).sum())
        deep += k["vertices"] / n > 3.0
        stars += (verts == NO_VERTEX).mean() > 0.5 and out["hdr"].any()
    in_atmosphere = sum(np.linalg.norm(c["pos"]) < sc.ATMOSPHERE for c, _ in rendered)
    in_shell = sum(sc.SHELL[0] <= np.linalg.norm(c["pos"]) < sc.SHELL[1] for c, _ in rendered)
    print("samples at the vertex limit %d, cases above 3 vertices per sample %d, star cases %d, in the atmosphere %d, in the shell %d"
          % (at_limit, deep, stars, in_atmosphere, in_shell))
    assert at_limit >= 1
    assert deep >= 8
    assert stars >= 3
    assert in_atmosphere >= 5
    assert in_shell >= 3


@pytest.mark.parametrize("what", ["clamp", "negative_scale", "topo_res_override", "wavelength_first", "wavelength_last"])
def test_the_switches_matter_where_they_are_set(rendered, lut_arrays, what):
    pick, back = {
        "clamp": (lambda c: c["clamp"], dict(clamp=False)),
        "negative_scale": (lambda c: c["land_height_scale"] < 0.0, dict(land_height_scale=sc.DEFAULT_SCALE)),
        "topo_res_override": (lambda c: c["topo_res_override"] != 0, dict(topo_res_override=0)),
        "wavelength_first": (lambda c: c["fixed_wavelength"] == sc.LAMBDA_FIRST, dict(fixed_wavelength=None)),
        "wavelength_last": (lambda c: c["fixed_wavelength"] == sc.LAMBDA_LAST, dict(fixed_wavelength=None)),
    }[what]
    # "one case": the first of the sweep's that sets the switch and sees what it acts on (a frame of sky alone has no map tap and no terrain)
    differs = []
    for case, out in [(c, out) for c, out in rendered if pick(c)][:6]:
        plain = copy.deepcopy(case)
        plain.update(back)
        if not np.array_equal(render(plain, lut_arrays)["hdr"], out["hdr"]):
            differs.append(case["id"])
            break
    assert differs, what
