"""The two coded outputs (JPEG and PNG) side by side on one context.  Their host state is two instances of one struct (csrc/de_context.h:
CodedOut) and their Python paths one implementation (renderer.py: _CodedFetch), so what a merge could get wrong is sharing: a guess, a counter or a
device cell that belongs to the other output.  Lagged fetches of both alternate over frames of different lengths — the first longer than either
output's first prefix, so that _end copies the whole of it from the cell's own device stream — and every file must equal the synchronous fetch of the
same frame byte for byte; each ring refuses a fifth _begin while the other is full."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
ERR_STATE = -4
W, H = 48, 40      # a context is a multiple of (16, 8): H = 8 mod 16, so the last MCU row is half padding.  Nine restart intervals at restart 1;
                   # 5800 filtered bytes: six deflate chunks of 1024, the last ragged


def _sums(k):
    """Frame k: noise (long files) where k is even, a flat field with one noisy column (short ones) where it is odd; never the same twice."""
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
    from digital_earth_amd import renderer as R
    r = R.Renderer((W, H), (0, 1, 0), texture_source="constant")
    r.copy_textures()
    r.set_pixels(3, "round")
    r.set_jpeg(100, 1)
    r.set_png(chunk_bytes=1024)
    frames = [_sums(k) for k in range(6)]
    want = []
    for s in frames:
        r.upload_hdr(s, 1)
        want.append((r.fetch_jpeg(), r.fetch_png()))
    for kind in (0, 1):
        lengths = [len(w[kind]) for w in want]
        assert all(a != b for a, b in zip(lengths, lengths[1:])), lengths      # a guess taken from the frame before is never exact
    assert len(want[0][0]) > 16 + 629 + W * H // 4 and len(want[0][1]) > 16 + 33 + H * (1 + 3 * W) // 4      # longer than the first prefixes
    got_j, got_p = [], []
    for k, s in enumerate(frames):
        r.upload_hdr(s, 1)
        j, p = r.fetch_jpeg(lag=2), r.fetch_png(lag=2)
        assert (j is None) == (p is None) == (k < 2)
        if j is not None:
            got_j.append(j), got_p.append(p)
    assert r._jp_in_flight == 2 and r._pn_in_flight == 2 and len(got_j) == len(got_p) == 4
    got_j += r.fetch_pending_jpeg(all_images=True)
    assert r._jp_in_flight == 0 and r._pn_in_flight == 2           # draining one ring leaves the other's counter alone
    got_p += r.fetch_pending_png(all_images=True)
    assert len(got_j) == len(got_p) == 6
    for k in range(6):
        _same(got_j[k], want[k][0], "the lagged JPEG of frame %d" % k)
        _same(got_p[k], want[k][1], "the lagged PNG of frame %d" % k)
    # each ring takes four and refuses a fifth, whatever the other holds
    L, h = r._lib, r._h
    for _ in range(4):
        assert L.de_fetch_jpeg_begin(h) == 0
        r._jp_in_flight += 1
    assert L.de_fetch_jpeg_begin(h) == ERR_STATE
    for _ in range(4):
        assert L.de_fetch_png_begin(h) == 0                        # the JPEG ring is full: the PNG ring is not
        r._pn_in_flight += 1
    assert L.de_fetch_png_begin(h) == ERR_STATE and L.de_fetch_jpeg_begin(h) == ERR_STATE
    files = r.fetch_pending_png(all_images=True)
    assert len(files) == 4 and L.de_fetch_jpeg_begin(h) == ERR_STATE      # an empty PNG ring frees no JPEG cell
    for f in files:
        _same(f, want[5][1], "a PNG of the full rings")
    files = r.fetch_pending_jpeg(all_images=True)
    assert len(files) == 4
    for f in files:
        _same(f, want[5][0], "a JPEG of the full rings")
    r.close()
