"""The four coded outputs (JPEG, PNG, OpenEXR and Radiance RGBE) side by side on one context.  Their host state is four instances of one
struct (csrc/de_context.h: CodedOut), their entry points one family over a format's descriptor (csrc/de_fetch.h: coded_fetch_begin ...) and their
Python paths one implementation (renderer.py: _CodedFetch), so what a merge could get wrong is sharing: a guess, a counter, a device cell or a
per-cell flag that belongs to another output.  Lagged fetches of all four alternate over frames of different lengths — the first longer than each
output's first prefix, so that _end copies the whole of it from the cell's own device stream — and every file must equal the synchronous fetch of the
same frame byte for byte; each ring refuses a fifth _begin whatever the other three hold.  The second test holds the per-cell flag of the two
scene-linear outputs (CodedOut::reads_pano): de_set_panorama waits for exactly the fetches of the scene-linear panorama, of either ring."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
ERR_STATE = -4
W, H = 48, 40      # a context is a multiple of (16, 8): H = 8 mod 16, so the last MCU row is half padding.  Nine restart intervals at restart 1;
                   # 5800 filtered bytes: six deflate chunks of 1024, the last ragged.  EXR: three blocks of 16, 16 and 8 lines, 11520 raw bytes
KINDS = ("jpeg", "png", "exr", "rgbe")
COUNTERS = ("_jp_in_flight", "_pn_in_flight", "_ex_in_flight", "_rg_in_flight")


def _sums(k):
    """Frame k: noise (long files) where k is even, a flat field with one noisy column (short ones) where it is odd; never the same twice.  On the CPU
    (exr_ref, rgbe_ref) the EXR files at zip and 1024-byte chunks are 11833, 3039, 11855, 3034, 11852, 3034 bytes against a first prefix of
    16 + 337 + 5760, the RGBE files 8098, 888, 8098, 896, 8097, 892 against 16 + 98 + 3840: zip compression serves, no output needs "none"."""
    rng = np.random.default_rng(50 + k)
    s = np.full((W, H, 3), 0.02 * (k + 1), F)
    cols = W if k % 2 == 0 else 1
    s[:cols] = (np.exp2(rng.uniform(-9.0, 3.0, (cols, H, 1))) * rng.uniform(0.3, 1.6, (cols, H, 3))).astype(F)
    return s


def _same(got, want, what):
    got, want = bytes(got), bytes(want)
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError("%s: %d bytes against %d, first difference at %d" % (what, len(got), len(want), first))


def test_alternating_lagged_fetches_share_nothing():
    import exr_ref as xr
    import rgbe_ref as rg
    from digital_earth_amd import renderer as R
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    r.copy_textures()
    r.set_pixels(3, "round")
    r.set_jpeg(100, 1)
    r.set_png(chunk_bytes=1024)
    r.set_exr(chunk_bytes=1024)
    r.set_rgbe()
    fetch = [getattr(r, "fetch_" + kind) for kind in KINDS]
    pending = [getattr(r, "fetch_pending_" + kind) for kind in KINDS]
    in_flight = lambda: [getattr(r, name) for name in COUNTERS]
    frames = [_sums(k) for k in range(6)]
    want = []
    for s in frames:
        r.upload_hdr(s, 1)
        want.append([f() for f in fetch])
    # the first prefixes of the four _begins: the framing and two bits per pixel; the front and a quarter of the filtered bytes; the front (header and
    # the offsets of three blocks) and half the raw bytes; the header and half the flat bytes
    first = (629 + W * H // 4, 33 + H * (1 + 3 * W) // 4, len(xr.front(W, H)) + 8 * 3 + W * H * 6 // 2, len(rg.front(W, H)) + 2 * W * H)
    for i, kind in enumerate(KINDS):
        lengths = [len(w[i]) for w in want]
        assert all(a != b for a, b in zip(lengths, lengths[1:])), (kind, lengths)      # a guess taken from the frame before is never exact
        assert lengths[0] > 16 + first[i], (kind, lengths[0], first[i])                  # longer than the first prefix
    got = [[] for _ in KINDS]
    for k, s in enumerate(frames):
        r.upload_hdr(s, 1)
        files = [f(lag=2) for f in fetch]
        assert all((f is None) == (k < 2) for f in files)
        if k >= 2:
            for i, f in enumerate(files):
                got[i].append(f)
    assert in_flight() == [2, 2, 2, 2] and all(len(g) == 4 for g in got)
    for i in range(4):
        got[i] += pending[i](all_images=True)
        assert in_flight() == [0] * (i + 1) + [2] * (3 - i)           # draining one ring leaves the others' counters alone
    for i, kind in enumerate(KINDS):
        assert len(got[i]) == 6
        for k in range(6):
            _same(got[i][k], want[k][i], "the lagged %s of frame %d" % (kind, k))
    # each ring takes four and refuses a fifth, whatever the other three hold
    L, h = r._lib, r._h
    begin = [getattr(L, "de_fetch_%s_begin" % kind) for kind in KINDS]
    for i in range(4):
        for _ in range(4):
            assert begin[i](h) == 0                                    # the rings before it are full: this one is not
            setattr(r, COUNTERS[i], getattr(r, COUNTERS[i]) + 1)
        assert [b(h) for b in begin[:i + 1]] == [ERR_STATE] * (i + 1)
    for i, kind in enumerate(KINDS):
        files = pending[i](all_images=True)
        assert len(files) == 4 and [b(h) for b in begin[i + 1:]] == [ERR_STATE] * (3 - i)      # an empty ring frees no other ring's cell
        for f in files:
            _same(f, want[5][i], "a %s of the full rings" % kind)
    r.close()


def test_set_panorama_waits_for_the_environment_fetches_of_either_ring():
    """One lagged EXR and one lagged RGBE fetch of the scene-linear panorama (face size 16, panorama 32 x 16, all six linear faces held): the
    panorama's settings are refused while either is in flight — after the EXR fetch has ended, because of the RGBE one — and taken once both have
    ended; both files equal their synchronous fetches."""
    from digital_earth_amd import _native
    from digital_earth_amd import renderer as R
    N, size = 16, (32, 16)
    r = R.Renderer((N, N), (0, 1, 0), texture_source="constant")
    r.copy_textures()
    r.set_exr(chunk_bytes=1024)
    r.set_rgbe()
    r.set_panorama(size, supersample=1)
    rng = np.random.default_rng(7)
    for face in range(6):
        r.upload_hdr((np.exp2(rng.uniform(-6.0, 3.0, (N, N, 1))) * rng.uniform(0.3, 1.6, (N, N, 3))).astype(F), 1)
        r.capture_environment_face(face)
    assert r.environment["captured"] == tuple(range(6)) and r.exr()["size"] == size and r.rgbe()["size"] == size
    want_exr, want_rgbe = r.fetch_exr(), r.fetch_rgbe()

    def refused(noun):
        with pytest.raises(_native.DigitalEarthError) as e:
            r.set_panorama(size, supersample=1)
        assert e.value.code == ERR_STATE and noun + " fetches are in flight" in str(e.value), str(e.value)

    assert r.fetch_exr(lag=1) is None and r.fetch_rgbe(lag=1) is None
    refused("EXR")
    got_exr = r.fetch_pending_exr()
    refused("RGBE")                                                    # the EXR ring is empty: the RGBE fetch still reads the linear faces
    got_rgbe = r.fetch_pending_rgbe()
    r.set_panorama(size, supersample=1)
    assert r.environment["captured"] == ()                             # taken: every call clears the faces
    _same(got_exr, want_exr, "the lagged EXR of the environment")
    _same(got_rgbe, want_rgbe, "the lagged RGBE of the environment")
    r.close()
