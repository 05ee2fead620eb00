"""The life of a context's memory (csrc/de_memory.h owns every allocation; tests/test_memory_host.py holds the owner type alone to its counts): one
process walks the transitions that replace, lend, give back and free buffers, three times over, with a borrower destroyed before its lender.

  share maps and LUTs into a second context -> the borrower gets one map, then the LUTs, of its own -> the lender trims its as-uploaded maps ->
  a 1-spp launch, then a 16-spp one (the record buffers grow) -> output scale off, then 2x (staging, ring cells and packed buffers grow; 8-bit pixels and
  a video frame fetched at both sizes, synchronously and lagged) -> set_look twice (fresh tables move in) -> debug_ordered_sum with 2, then 3 parts (the
  gather buffer grows) -> v6_cu_withhold through set_tuning (the launch streams and the cold records are made again)

Every call must succeed; the borrower's picture must equal the lender's bit for bit for equal parameters and seed, while it borrows and after it owns
again; cycle 3's pictures must equal cycle 1's; and a lender is not destroyed while a borrower lives (DE_ERR_STATE).  In the second cycle the borrower
ends up owning every map (the loan is given back while both contexts live), in the others it is destroyed still holding views of six maps.  Nothing
is asserted about device-wide free memory: the device is shared.  64 x 32, synthetic 256 x 128 maps: a few seconds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERR_STATE = -4
W, H = 64, 32
BIG = (128, 64)
CLOUDS = 2


def _renderer(R):
    r = R.Renderer((W, H), (0, 1, 0), texture_source="synthetic", texture_size=(256, 128), seed=7)
    r.set_fov(0.42)
    r.set_pixels(3, "round")
    r.set_video("nv12")
    return r


def _frame(r):
    """A 1-spp launch, then a 16-spp one: the record buffers of the launch slots grow between the two."""
    r.reset_framebuffer()
    r.accumulate(1)
    r.accumulate(16)
    return [r.fetch_hdr(), r.fetch_image()]


def _outputs(r):
    """The image, the pixels and a video frame, synchronously and through the rings, at the size that is set."""
    out = [r.fetch_image(), r.fetch_pixels(), r.fetch_video()]
    for fetch, pending in ((r.fetch_image, {}), (r.fetch_pixels, dict(pixels=True)), (r.fetch_video, dict(video=True))):
        assert fetch(lag=1) is None
        out.append(fetch(lag=1))
        out.append(r.fetch_pending(**pending))
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        assert (g.view(np.uint8) == w.view(np.uint8)).all(), (what, k)


def _cycle(R, cycle):
    from digital_earth_amd import _native, cube as cube_mod
    lender, borrower = _renderer(R), _renderer(R)
    lender.copy_textures()
    seen = []

    def both(fn, what):
        got, want = fn(borrower), fn(lender)
        _same(got, want, "cycle %d, %s: the borrower against the lender" % (cycle, what))
        seen.extend(want)

    borrower.share_textures_from(lender)
    assert lender._lib.de_destroy(lender._h) == ERR_STATE      # refused: a borrower lives
    both(_frame, "borrowing everything")
    borrower.copy_texture(CLOUDS)                               # one map of its own (the same plan: the same texels)
    both(_frame, "owning the cloud map")
    cie, s2s, o3, crf = borrower._luts                          # LUTs of its own
    _native.check(borrower._lib.de_upload_luts(borrower._h, cie.ctypes.data, s2s.ctypes.data, o3.ctypes.data, crf.ctypes.data, crf.shape[1]))
    both(_frame, "owning the cloud map and the LUTs")
    lender.trim_textures()
    assert lender._lib.de_destroy(lender._h) == ERR_STATE      # six maps are still on loan
    if cycle == 1:                                              # every map its own: the loan goes back
        for slot in range(7):
            if slot != CLOUDS:
                borrower.copy_texture(slot)
    both(_frame, "after the lender's trim")

    both(_outputs, "outputs at the native size")
    for r in (lender, borrower):
        r.set_output_scale(BIG)
    both(_outputs, "outputs at twice the size")
    both(_outputs, "outputs at twice the size, buffers held")
    for r in (lender, borrower):
        r.set_output_scale(None, on=False)
    both(_outputs, "outputs at the native size, below the capacity")

    grade = np.clip(np.frombuffer(cube_mod.identity(5).table, dtype=np.float32) ** 0.8, 0, 1).astype(np.float32)
    for table in (cube_mod.identity(9), cube_mod.Cube("3d", 5, grade)):      # twice: the second upload replaces the first one's tables
        for r in (lender, borrower):
            r.set_look(cube=table)
        both(lambda r: [r.fetch_image(), r.fetch_pixels()], "look, %d^3" % table.size)
    for r in (lender, borrower):
        r.set_look(enabled=False)

    rng = np.random.default_rng(5)
    parts = rng.random((3, W, H, 3), dtype=np.float32)
    for n in (2, 3):                                            # the gather buffer grows
        both(lambda r: [r.debug_ordered_sum(parts[:n], root=0, out_of_place=True)], "ordered sum of %d parts" % n)

    for withhold in (1, 0):                                     # the launch streams and the cold records are made again
        for r in (lender, borrower):
            t = r.tuning()
            t.v6_cu_withhold = withhold
            r.set_tuning(t)
        both(_frame, "v6_cu_withhold = %d" % withhold)

    if cycle != 1:
        assert lender._lib.de_destroy(lender._h) == ERR_STATE  # still refused at the end of the walk
    borrower.close()                                            # the borrower before its lender: its views free nothing
    seen.extend(_frame(lender))                                 # the lender's blocks are alive and whole
    lender.close()
    return seen


def test_ownership_transitions_three_times_over():
    from digital_earth_amd import renderer as R
    first = _cycle(R, 0)
    _cycle(R, 1)
    third = _cycle(R, 2)
    _same(third, first, "cycle 3 against cycle 1")
    assert any(np.asarray(a).any() for a in first)              # pictures, not zeros
