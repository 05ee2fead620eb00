"""The loops that only run at production frame sizes.  The other GPU tests use frames of 16 x 8 to 512 x 256, at which four kernels never take the
second trip of a loop that a 1920 x 1080 frame takes every time:
  A  meter_hist_kernel's grid-stride loop (more than 512 x 256 items) and meter_solve_kernel's unrolled row summation (61 partial rows or more)
  B  adaptive_compact_kernel's walk over the active list in chunks of 1024 entries, `base` carried across chunks
  C  jpeg_scan_kernel with more than 1024 restart intervals: several intervals per thread, a ragged last owner, threads that own none
  D  ordered_sum_kernel's float4 stride loop past one item per launched thread
Every test first asserts, from the launch arithmetic restated on the host, that its shape reaches the trip it is there for, so that a later change of
a constant makes it fail instead of pass empty; then it holds the kernel to the restatement the small sizes are held to (tests/exposure_f64.py, the
definitions of tests/test_gpu_adaptive.py, tests/jpeg_ref.py, numpy's f32 sum in rank order) with the same bounds."""
import numpy as np
import pytest

import exposure_f64 as ae
import jpeg_cases as jc
import test_gpu_adaptive as ad
import test_gpu_exposure as ex

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- A. the auto-exposure meter
MW, MH = 1024, 520
AE_MAX_WG, AE_WG_THREADS = 512, 256      # csrc/exposure_kernels.hip and run_meter (csrc/de_display.h): at most 512 workgroups of 256 items, one partial row each
METER_SPPS = (1, 3)


def _full_width(h):
    y0 = min(3, MH - h)
    return (0, y0, MW, y0 + h)


# region -> (n_rows, trips of the unrolled loop per row group 0 .. 3, whether the stride loop takes a second trip).  Full-width regions have 256 items
# per image row, so n_rows = min(h, 512): the last height with no unrolled trip, the heights at which row groups 0 to 3 enter it one by one, one row past
# that, the last height of one trip everywhere, two trips for row group 0 and for all, the cap, the first row past the cap, the whole frame; then
# unaligned columns (the first and the last group of every row are partly outside) and an item count that is no multiple of 64 (a ragged last wave, in
# the second trip).
METER_CASES = [
    (_full_width(60), (60, (0, 0, 0, 0), False)),
    (_full_width(61), (61, (1, 0, 0, 0), False)),
    (_full_width(62), (62, (1, 1, 0, 0), False)),
    (_full_width(63), (63, (1, 1, 1, 0), False)),
    (_full_width(64), (64, (1, 1, 1, 1), False)),
    (_full_width(65), (65, (1, 1, 1, 1), False)),
    (_full_width(124), (124, (1, 1, 1, 1), False)),
    (_full_width(125), (125, (2, 1, 1, 1), False)),
    (_full_width(128), (128, (2, 2, 2, 2), False)),
    (_full_width(512), (512, (8, 8, 8, 8), False)),
    (_full_width(513), (512, (8, 8, 8, 8), True)),
    (_full_width(520), (512, (8, 8, 8, 8), True)),
    ((3, 1, MW - 2, MH - 1), (512, (8, 8, 8, 8), True)),
    ((4, 0, MW, 515), (512, (8, 8, 8, 8), True)),
]


def _meter_launch(region):
    """run_meter's arithmetic: (items, n_rows, trips of `for (; r + 60 < n_rows; r += 64)` from r = rg for the four row groups, items > 512 * 256)."""
    x0, y0, x1, y1 = region
    gx0 = x0 >> 2
    gw = ((x1 + 3) >> 2) - gx0
    items = gw * (y1 - y0)
    n_rows = min(-(-items // AE_WG_THREADS), AE_MAX_WG)
    trips = tuple(len(range(rg, n_rows - 60, 64)) for rg in range(4))
    return items, n_rows, trips, items > AE_MAX_WG * AE_WG_THREADS


_METER_INPUTS = {}


def _meter_inputs():
    """name -> (W, H, 3) sums: the mixed image of tests/test_gpu_exposure.py's generator with a few NaN and infinite sums planted, and its constant one
    (all 64 lanes of every wave in one bin: ae_count's leader path, added 512 rows deep)."""
    if not _METER_INPUTS:
        made = ex._inputs(MW, MH)
        mixed = made["mixed"].copy()
        mixed[5::97, 7::89, 1] = np.nan
        mixed[11::101, 3::83] = np.inf
        mixed.flags.writeable = False
        with np.errstate(all="ignore"):
            Y = ae.luminance(mixed)
        whole = ae.meter(mixed, 1)
        # every class of pixel is there: metered, below 2^-24, clipped, exact zeros, negative and NaN luminances
        assert whole["metered"] > 0 and whole["below"] > 0 and whole["clipped"] > 0 and (np.count_nonzero(whole["histogram"]) == ae.BINS)
        assert (Y == 0).any() and (Y < 0).any() and np.isnan(Y).any() and np.isposinf(Y).any()
        _METER_INPUTS.update(mixed=mixed, constant=made["constant"])
    return _METER_INPUTS


@pytest.fixture(scope="module")
def meter_ctx(R):
    r = R.Renderer((MW, MH), (0, 1, 0), texture_source="constant")
    r.copy_textures()
    yield r
    r.close()


@pytest.mark.parametrize("case", METER_CASES, ids=["%d-%d-%d-%d" % region for region, _ in METER_CASES])
def test_meter_beyond_one_trip_equals_the_restatement(meter_ctx, case):
    """Histogram, n, below and clipped exactly; EV, target and mean within the 2 ulp of test_ev_within_2_ulp_of_the_f64_restatement."""
    region, (n_rows, trips, second_trip) = case
    items, got_rows, got_trips, got_second = _meter_launch(region)
    assert got_rows == n_rows
    assert got_trips == trips and [rg + 60 < n_rows for rg in range(4)] == [t > 0 for t in trips]
    assert got_second == second_trip == (items > 512 * 256)
    if region == (4, 0, MW, 515):
        assert items % 64 != 0
    x0, y0, x1, y1 = region
    area = (x1 - x0) * (y1 - y0)
    r = meter_ctx
    manual = float(r.exposure[None])
    for spp in METER_SPPS:
        for name, sums in _meter_inputs().items():
            r.set_auto_exposure(True, region=region)          # clears the state: every metering is a first one
            m = ex._show(r, sums, spp)
            want_h = ae.meter(sums, spp, region=region)
            ex._same_histogram(m, want_h)
            assert m["metered"] + m["below"] == area
            if name == "constant":
                assert m["histogram"].max() == area
            want = ae.Meter(region=region).update(want_h["histogram"], manual_exposure=manual)
            assert m["valid"] and want["valid"]
            d = [ae.ulps_f32(m[key], want[key]) for key in ("ev", "ev_target", "mean_log2")]
            print("%s %s spp %d: %d rows, ev %.6f target %.6f mean %.6f, ulps %s" % (region, name, spp, n_rows, m["ev"], m["ev_target"], m["mean_log2"], d))
            assert max(d) <= 2.0, (name, spp, d, m["ev"], want["ev"])
    r.set_auto_exposure(False)


def test_meter_cases_cover_what_they_are_there_for():
    """The sweep as a whole, on the host: a height with no unrolled trip, every row group entering alone, one and two trips, both sides of the cap."""
    launches = [_meter_launch(region) for region, _ in METER_CASES]
    assert [l[1] for l in launches[:12]] == [60, 61, 62, 63, 64, 65, 124, 125, 128, 512, 512, 512]
    assert {l[2] for l in launches} >= {(0, 0, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 1), (2, 1, 1, 1), (2, 2, 2, 2)}
    assert {l[3] for l in launches} == {False, True}
    assert launches[10][0] == 512 * 256 + 256 and launches[9][0] == 512 * 256      # the first row past the cap, and the cap itself
    assert (launches[12][0], launches[13][0]) == (256 * 518, 255 * 515)


# ---------------------------------------------------------------- B. the adaptive compaction
AW, AH = 528, 256                     # 66 x 32 = 2112 tiles: two full chunks of 1024 list entries and a ragged one of 64
COMPACT_CHUNK = 1024                  # adaptive_compact_kernel (csrc/adaptive_kernels.hip): one workgroup of 1024 threads, one list entry each per chunk
A_MIN, A_ROUND, A_MAX = 4, 4, 16
A_TAUS = ad.TAUS


def _compactions(counts):
    """The compactions of an adaptive frame, reconstructed from its final tile counts: per round (count reached, the list it compacts, which entries
    stay).  A list is ascending in the tile id ty * tiles_x + tx, so the list of the round that reached n holds the tiles whose final count is at
    least n, and the entries that stay are those whose final count exceeds n."""
    ids = np.ascontiguousarray(counts.T).ravel()      # tile_spp() is (W/8, H/8)
    out = []
    for n in range(A_ROUND, A_MAX + 1, A_ROUND):
        active = np.nonzero(ids >= n)[0]
        out.append((n, active, ids[active] > n))
    return out


def _chunk_facts(counts):
    """Per round: (count reached, list entries, chunks that hold both kept and dropped entries, whether a kept entry lies in a later chunk than a dropped one)."""
    facts = []
    for n, active, kept in _compactions(counts):
        chunk = np.arange(len(active)) // COMPACT_CHUNK
        mixed = [c for c in np.unique(chunk) if kept[chunk == c].any() and not kept[chunk == c].all()]
        later = bool(kept.any() and not kept.all() and chunk[kept].max() > chunk[~kept].min())
        facts.append((n, len(active), len(mixed), later))
    return facts


def _reaches_the_chunk_boundaries(counts):
    return any(entries > COMPACT_CHUNK and mixed >= 2 and later for _, entries, mixed, later in _chunk_facts(counts))


@pytest.fixture(scope="module")
def adaptive_ctx(R):
    r = ad._renderer(R, AW, AH)
    yield r
    r.close()


_ADAPTIVE = {}


def _adaptive_frame(r):
    """The first threshold of the list whose frame compacts a list of more than 1024 entries with kept and dropped tiles on both sides of a chunk
    boundary: (tau, counts, hdr, image), made once."""
    if not _ADAPTIVE:
        seen = []
        for tau in A_TAUS:
            counts, hdr, img, info = ad._adaptive(r, tau, A_MAX, A_MIN, A_ROUND)
            seen.append((tau, _chunk_facts(counts)))
            if _reaches_the_chunk_boundaries(counts):
                _ADAPTIVE.update(frame=(tau, counts, hdr, img, info))
                break
        else:
            pytest.fail("no threshold compacts a list of more than %d entries with kept and dropped tiles in two chunks: %s" % (COMPACT_CHUNK, seen))
    return _ADAPTIVE["frame"]


def test_compaction_across_chunks_every_tile_equals_the_uniform_frame_at_its_count(adaptive_ctx):
    r = adaptive_ctx
    assert (AW // 8) * (AH // 8) == 2 * COMPACT_CHUNK + 64
    tau, counts, hdr, img, info = _adaptive_frame(r)
    facts = _chunk_facts(counts)
    print("tau %s: (count, list entries, chunks with kept and dropped, kept behind dropped) %s" % (tau, facts))
    assert any(entries > COMPACT_CHUNK for _, entries, _, _ in facts)
    assert any(entries > COMPACT_CHUNK and mixed >= 2 for _, entries, mixed, _ in facts)
    assert any(entries > COMPACT_CHUNK and mixed >= 2 and later for _, entries, mixed, later in facts)
    assert counts.shape == (AW // 8, AH // 8) and counts.dtype == np.int32
    assert set(np.unique(counts)) <= {4, 8, 12, 16} and len(np.unique(counts)) >= 2
    assert info["pixel_samples"] == 64 * int(counts.sum())
    for n in np.unique(counts):
        u_hdr, u_img = ad._uniform(r, int(n))
        m = ad._pixel_mask(counts, n)
        assert (_bits(hdr)[m] == _bits(u_hdr)[m]).all(), (tau, n)
        assert (_bits(img)[m] == _bits(u_img)[m]).all(), (tau, n)


def test_compaction_across_chunks_every_decision_follows_the_definition(R, adaptive_ctx):
    """test_every_decision_follows_the_definition at 2112 tiles: after every round, the tiles the compaction kept are the tiles the definition keeps
    (margins within 1e-4 exempt), and the next list holds exactly them."""
    r = adaptive_ctx
    tau, counts, _, _, _ = _adaptive_frame(r)
    assert _reaches_the_chunk_boundaries(counts)
    floor = R.ADAPTIVE_FLOOR
    r.reset_framebuffer()
    snaps = []
    while True:
        active = r.accumulate_adaptive(tau, A_MAX, min_spp=A_MIN, round_spp=A_ROUND)
        snaps.append((r.tile_spp(), r.fetch_hdr(), r.adaptive_moments(), active))
        if active == 0:
            break
    assert (snaps[-1][0] == counts).all()
    checked = 0
    for k, (c, s1, s2, active) in enumerate(snaps):
        n = int(c.max())
        nxt = snaps[k + 1][0] if k + 1 < len(snaps) else c
        kept = nxt > c
        assert int(kept.sum()) == active
        was_active = c == n
        assert not (kept & ~was_active).any()
        if n >= A_MAX:
            assert active == 0
            continue
        stays, margin = ad._decisions(s1, s2, n, tau, floor)
        decided = was_active & (margin > 1e-4)
        assert (kept[decided] == stays[decided]).all(), (k, n, int((kept[decided] != stays[decided]).sum()))
        checked += int(decided.sum())
    assert checked > COMPACT_CHUNK


# ---------------------------------------------------------------- C. the JPEG scan
# (W, H, restart) -> (intervals, intervals per owning thread, threads that own none, intervals of the last owner)
SCAN_EXPECTED = {(528, 528, 1): (1089, 2, 479, 1), (544, 1040, 1): (2210, 3, 287, 2)}


@pytest.fixture(scope="module")
def jpeg_ctx(R):
    r = R.Renderer((64, 32), (0, 1, 0), texture_source="constant")      # de_debug_jpeg encodes an image of any even size
    r.copy_textures()
    yield r
    r.close()


@pytest.mark.parametrize("name", jc.LARGE_INPUTS)
@pytest.mark.parametrize("size", jc.LARGE_SIZES, ids=lambda s: "%dx%d-r%d" % s)
def test_scan_with_several_intervals_per_thread_equals_the_restatement(jpeg_ctx, size, name):
    w, h, restart = size
    intervals, chunk, idle, last = SCAN_EXPECTED[size]
    assert restart == 1 and intervals == ((w + 15) // 16) * ((h + 15) // 16) > jc.SCAN_THREADS
    assert jc.scan_geometry(intervals) == (chunk, jc.SCAN_THREADS - idle, idle, last)
    assert chunk >= 2 and idle > 0 and intervals % chunk != 0 and 0 < last < chunk      # a ragged last owner, and threads whose `lo` is past the end
    jc.check_precondition(name, w, h, restart)
    want, st, _ = jc.reference(name, w, h, restart)
    assert st["intervals"] == intervals
    got = jpeg_ctx.debug_jpeg(jc.image(name, w, h), quality=jc.QUALITY[name], restart=restart)
    got, want = bytes(got), bytes(want)
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("%s %s: %d bytes against %d, first difference at %d" % (name, size, len(got), len(want), first))


def test_scan_cases_have_chunks_of_two_and_three():
    assert sorted(SCAN_EXPECTED) == sorted(jc.LARGE_SIZES)
    assert sorted(v[1] for v in SCAN_EXPECTED.values()) == [2, 3]


# ---------------------------------------------------------------- D. the ordered sum
SW, SH = 1024, 688                    # 704 512 pixels = 528 384 float4 against the 524 288 threads of a 256-CU part
SUM_WG_PER_CU, SUM_WG_THREADS = 8, 256      # launch_ordered_sum (csrc/de_rccl.h)
SUM_MAX_PARTS = 16


def _device_cus():
    """The CU count of device 0 from the runtime the library itself runs on: the multiProcessorCount that de_create reads into the context (the
    library has no getter for it).  63 is hipDeviceAttributeMultiprocessorCount of hip_runtime_api.h."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    n = ctypes.c_int(0)
    assert hip.hipDeviceGetAttribute(ctypes.byref(n), ctypes.c_int(63), ctypes.c_int(0)) == 0 and 0 < n.value <= 4096, n.value
    return n.value


def _sum_height(n_cus):
    """688, or the smallest height above it in steps of 8 at which the float4 loop takes a second trip on a part with more CUs."""
    h = SH
    while SW * h * 3 // 4 <= n_cus * SUM_WG_PER_CU * SUM_WG_THREADS:
        h += 8
    return h


@pytest.fixture(scope="module")
def sum_ctx(R):
    n_cus = _device_cus()
    r = R.Renderer((SW, _sum_height(n_cus)), (0, 1, 0), texture_source="constant")
    r.copy_textures()
    yield r, n_cus
    r.close()


_SUM_PARTS = {}


def _sum_parts(shape):
    """Sixteen parts whose sum depends on the order: magnitudes spread over 2^20, signs mixed.  Made once, never written to."""
    if shape not in _SUM_PARTS:
        rng = np.random.default_rng(20)
        parts = []
        for _ in range(SUM_MAX_PARTS):
            p = (rng.standard_normal(shape) * np.exp2(rng.integers(-10, 11, size=shape))).astype(np.float32)
            p.flags.writeable = False
            parts.append(p)
        _SUM_PARTS[shape] = parts
    return _SUM_PARTS[shape]


@pytest.mark.parametrize("out_of_place", [False, True], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("n_parts,root", [(2, 0), (2, 1), (3, 0), (3, 1), (16, 0), (16, 7)])
def test_ordered_sum_beyond_one_item_per_thread(sum_ctx, n_parts, root, out_of_place):
    """((p0 + p1) + p2) + ... in f32, bit for bit, where the float4 loop takes a second trip."""
    r, n_cus = sum_ctx
    W, H = r.image_res
    threads = n_cus * SUM_WG_PER_CU * SUM_WG_THREADS
    n4 = W * H * 3 // 4
    assert W * H * 3 % 4 == 0 and threads < n4 <= 2 * threads      # some threads take a second trip and some do not; no scalar tail
    assert (n_cus != 256) or (W, H) == (SW, SH)
    parts = _sum_parts((W, H, 3))[:n_parts]
    want = parts[0]
    for p in parts[1:]:
        want = want + p
    other = parts[-1]
    for p in parts[-2::-1]:
        other = other + p
    # the inputs tell the orders apart (two parts cannot: a + b = b + a), and do so in the second trip's items too ([H][W][3] on the device)
    differs = np.ascontiguousarray((_bits(other) != _bits(want)).transpose(1, 0, 2)).ravel()
    assert n_parts == 2 or (differs[:4 * threads].any() and differs[4 * threads:].any())
    assert want.dtype == np.float32
    got = r.debug_ordered_sum(parts, root=root, out_of_place=out_of_place)
    if out_of_place:
        r.set_display_source(None)
    wrong = np.ascontiguousarray((_bits(got) != _bits(want)).transpose(1, 0, 2)).ravel()
    assert not wrong.any(), "%d floats differ, the first at %d (second trip from %d)" % (wrong.sum(), int(np.argmax(wrong)), 4 * threads)
