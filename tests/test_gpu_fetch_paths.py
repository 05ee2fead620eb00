"""The host-copy paths of every fetch (csrc/de_fetch.h) on the GPU: one staging buffer, one device buffer, one ring and one conversion counter serve
the float image, the 8-bit pixels, the video frames and the HDR pixels.  A context that fetches LAGGED is held to a synchronous twin, byte for byte,
through a sequence that crosses every edge of a buffer's life that the shared code owns: first use, growth of every ring cell, staging buffer and device
buffer with the output size, use at a size below the capacity, three rings in flight side by side, release.  What the bytes ARE is the other test
files' business (test_gpu_pixels.py, test_gpu_video.py, test_gpu_output_scale.py); the HDR pixels, which have no ring, are held to the transform
kernel and the packed restatement (tests/hdr_output_ref.py) at native size, enlarged, and native again.

64 x 32 with synthetic maps, one sample per frame: every frame differs from the one before (the sums progress), so a frame handed out of order, a
stale cell or a copy of the wrong length shows."""
import ctypes

import numpy as np
import pytest

import hdr_output_ref as ho

pytestmark = pytest.mark.gpu

ERR_STATE = -4
W, H = 64, 32
BIG = (128, 64)
U8 = ctypes.POINTER(ctypes.c_uint8)

# a ringed output: the Renderer's fetch, fetch_pending's keyword, the entry points' stem and what sets its format (3 channels: size != capacity at every size)
OUTPUTS = {
    "image": dict(fetch="fetch_image", pending={}, stem="de_fetch_image", ctype=ctypes.c_float, setup=lambda r: None),
    "pixels": dict(fetch="fetch_pixels", pending=dict(pixels=True), stem="de_fetch_pixels", ctype=ctypes.c_uint8, setup=lambda r: r.set_pixels(3, "round")),
    "video": dict(fetch="fetch_video", pending=dict(video=True), stem="de_fetch_videoframe", ctype=ctypes.c_uint8, setup=lambda r: r.set_video("i010")),
}


@pytest.fixture(scope="module")
def R():
    from digital_earth_amd import renderer
    return renderer


def _renderer(R):
    r = R.Renderer((W, H), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512), seed=17)
    r.set_fov(0.42)
    r.copy_textures()
    for o in OUTPUTS.values():
        o["setup"](r)
    return r


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = _bytes(got) != _bytes(want)
    assert not diff.any(), (what, int(diff.sum()), np.flatnonzero(diff)[:6].tolist())


def _lagged_loop(lagged, twin, o, lag, frames, what):
    """`frames` frames of accumulate(1) + fetch(lag) against the twin's accumulate(1) + fetch(); then the drain.  Returns the twin's newest frame."""
    got, want = [], []
    for _ in range(frames):
        lagged.accumulate(1)
        got.append(getattr(lagged, o["fetch"])(lag=lag))
        twin.accumulate(1)
        want.append(getattr(twin, o["fetch"])())
    assert all(g is None for g in got[:lag]), what
    rest = lagged.fetch_pending(all_images=True, **o["pending"])
    assert len(rest) == lag and lagged.fetch_pending(**o["pending"]) is None, what
    seq = got[lag:] + rest
    assert len(seq) == frames
    for k in range(frames):
        _same(seq[k], want[k], (what, k))
    assert (_bytes(want[0]) != _bytes(want[-1])).any(), what      # the frames do differ: an order could show
    return want[-1]


@pytest.mark.parametrize("name", list(OUTPUTS))
def test_lagged_context_equals_its_synchronous_twin_through_every_buffer_edge(R, name):
    o = OUTPUTS[name]
    lagged, twin = _renderer(R), _renderer(R)
    L, h = lagged._lib, lagged._h
    # (a) first use of the ring: a lag-3 loop of six frames at the native size, drained
    native = _lagged_loop(lagged, twin, o, 3, 6, "a")
    # (b) the output size grows: every ring cell and the device buffer regrow; a lag-2 loop of five frames, drained
    lagged.set_output_scale(BIG); twin.set_output_scale(BIG)
    big = _lagged_loop(lagged, twin, o, 2, 5, "b")
    assert big.nbytes == 4 * native.nbytes
    # (c) back at the native size the buffers are larger than the frame: `size` bytes of `capacity`.  The staging buffer's first use, too.
    lagged.set_output_scale(on=False); twin.set_output_scale(on=False)
    lagged.accumulate(1); twin.accumulate(1)
    want = getattr(twin, o["fetch"])()
    view = getattr(lagged, o["fetch"])(copy=False)
    assert not view.flags.writeable and view.nbytes == native.nbytes
    _same(np.array(view), want, "c view")
    _same(getattr(lagged, o["fetch"])(), want, "c copy")
    held = np.array(view)
    # (d) two fetches of this ring in flight; the other two rings still take four begins each, refuse the fifth and hand their frames out in order
    refs = {n: [] for n in OUTPUTS}

    def begin(n):
        lagged.accumulate(1); twin.accumulate(1)
        assert getattr(L, OUTPUTS[n]["stem"] + "_begin")(h) == 0, n
        refs[n].append(getattr(twin, OUTPUTS[n]["fetch"])())

    def end(n, k):
        ptr = ctypes.POINTER(OUTPUTS[n]["ctype"])()
        assert getattr(L, OUTPUTS[n]["stem"] + "_end")(h, ctypes.byref(ptr)) == 0, (n, k)
        want = refs[n][k]
        got = np.ctypeslib.as_array(ctypes.cast(ptr, U8), shape=(want.nbytes,))
        assert (got == _bytes(want)).all(), (n, k)

    for _ in range(2):
        begin(name)
    others = [n for n in OUTPUTS if n != name]
    for k in range(4):
        for n in others:      # the other two rings fill side by side
            begin(n)
    for n in others:
        assert getattr(L, OUTPUTS[n]["stem"] + "_begin")(h) == ERR_STATE, n
    for n in reversed(others):
        for k in range(4):
            end(n, k)
    for k in range(2):
        end(name, k)
    for n in OUTPUTS:
        ptr = ctypes.POINTER(OUTPUTS[n]["ctype"])()
        assert getattr(L, OUTPUTS[n]["stem"] + "_end")(h, ctypes.byref(ptr)) == ERR_STATE, n
    _same(np.array(view), held, "the staging buffer is no ring cell: the view of (c) still holds its frame")
    # (e) release: refused while the view of (c) is referenced, done once it is dropped
    with pytest.raises(RuntimeError):
        lagged.close()
    del view
    lagged.close()
    twin.close()


def test_hdr_pixels_at_native_size_enlarged_and_native_again(R):
    """No ring: the staging and the device buffer alone — first use, growth, use below the capacity — and the conversion counter, through an animated
    dither: the three fetches are conversions 0, 1 and 2."""
    r = _renderer(R)
    r.accumulate(1)
    config = dict(peak_nits=1000.0, gamut="rec2020", transfer="pq")
    r.set_hdr_output(True, pixel_format="rgb16", mode="dither", seed=5, animate=True, **config)
    sqrt = lambda x: r.debug_math(8, x)      # the device's own de_sqrt and de_pow: the vignette's distance, the exposure's 2^ev
    scale = float(r.debug_math(6, np.array([2.0], np.float32), np.array([2.5], np.float32))[0])
    vignette = (r.vignette_strength, r.vignette_radius) + tuple(r.vignette_center)
    signal = r.debug_hdr_transform(ho.display_linear(r.fetch_hdr(), 1, scale, vignette, sqrt=sqrt), **config)
    enlarged = r.debug_output_scale(signal, BIG)
    for phase, (size, image) in enumerate(((None, signal), (BIG, enlarged), (None, signal))):
        r.set_output_scale(size)
        px = r.fetch_hdr_pixels()
        want = ho.pack(image, "rgb16", "dither", seed=5, phase=phase)
        assert px.dtype == np.uint16 and px.shape == want.shape == (image.shape[1], image.shape[0], 3), (phase, px.shape)
        assert (px == want).all(), (phase, int((px != want).sum()))
        assert r.hdr_output["last_phase"] == phase
    r.close()
