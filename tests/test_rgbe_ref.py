"""The Radiance HDR output's restatement on the CPU (tests/rgbe_ref.py, include/digital_earth_rgbe.h): the header's known answers, every case file
decoded again by digital_earth_amd/rgbe.py to within the stated step, the proven size bound on every case, and a decoder written here, apart from
both, that agrees with rgbe.py."""
import numpy as np
import pytest

import rgbe_cases as gc
import rgbe_ref as gr
from digital_earth_amd import rgbe

F = np.float32


def _ten_line_decoder(data):
    """(H, W, 4) uint8 of a file of this output, written from the format alone."""
    head, _, body = data.partition(b"\n\n")
    res, _, body = body.partition(b"\n")
    H, W = int(res.split()[1]), int(res.split()[3])
    if not (8 <= W <= 32767 and body[:2] == b"\x02\x02"):
        return np.frombuffer(body, np.uint8).reshape(H, W, 4)
    flat, at = [], 0
    while at < len(body):
        if len(flat) % (4 * W) == 0:
            at += 4                                                 # a row's 02 02 hi lo
        n = body[at]
        flat += [body[at + 1]] * (n - 128) if n > 128 else list(body[at + 1:at + 1 + n])
        at += 2 if n > 128 else 1 + n
    return np.array(flat, np.uint8).reshape(H, 4, W).transpose(0, 2, 1)


@pytest.mark.parametrize("value, rounding, want", gc.KNOWN)
def test_known_answers(value, rounding, want):
    assert gr.pixels(np.array([value], F), 1.0, rounding).tobytes().hex().upper() == want
    assert rgbe._encode_pixels(np.array([value], F), rounding).tobytes().hex().upper() == want      # the host writer, which works in floats


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_case_decodes_within_its_step_and_its_bound(name):
    image, rle, rounding, scale = gc.CASES[name]
    H, W = image.shape[:2]
    data = gc.encoded(name)
    assert len(data) <= gr.capacity(W, H, rle, scale)
    if gr.is_rle(W, rle):                                           # plane by plane: W + ceil(W / 128)
        px = gr.pixels(image, scale, rounding)
        assert max(len(gr.encode_plane(px[y, :, c])) for y in range(H) for c in range(4)) <= gr.plane_bound(W)
    stored, info = rgbe.decode(data)
    assert (info["width"], info["height"]) == (W, H) and set(info["rows"]) == {"rle" if gr.is_rle(W, rle) else "flat"}
    assert np.array_equal(stored, gr.pixels(image, scale, rounding)) and np.array_equal(stored, _ten_line_decoder(data))
    assert info["exposure"] == float(F(scale)) and info["primaries"] == tuple(float(x) for x in gr.PRIMARIES.split())
    assert (b"EXPOSURE=0.25" in info["lines"]) == (scale == 0.25) and any(l.startswith(b"EXPOSURE=") for l in info["lines"]) == (scale != 1.0)
    # the values: the source as the format can hold it (NaN and negatives 0, the clamp), against both decoding conventions
    src = (image * F(scale)).astype(np.float64)
    src = np.where(np.isnan(src) | (src < 0), 0.0, np.minimum(src, 255 * 2.0 ** 119))
    step = np.ldexp(1.0, stored[..., 3:4].astype(np.int32) - 136)   # 2^(e - 8)
    lit = stored[..., 3:4] != 0
    low, mid = rgbe.read(data)[0].astype(np.float64), rgbe.read(data, half_step=True)[0].astype(np.float64)
    assert (np.abs(low - src) <= step)[np.broadcast_to(lit, src.shape)].all()
    if rounding == "round":
        assert (np.abs(low - src) <= step / 2)[np.broadcast_to(lit, src.shape)].all()
    else:
        assert ((low <= src) & (np.abs(mid - src) <= step / 2))[np.broadcast_to(lit, src.shape)].all()
    assert (src.max(axis=-1)[~lit[..., 0]] < 1e-32).all() and (low[~np.broadcast_to(lit, src.shape)] == 0).all()
    assert rgbe.write(None, image, rle=rle, rounding=rounding, scale=scale) == data      # the host writer makes the same file


def test_reader_refuses_what_it_does_not_read(tmp_path):
    data = gc.encoded("w009_h1")
    path = tmp_path / "x.hdr"
    path.write_bytes(data)
    assert np.array_equal(rgbe.read(str(path))[0], rgbe.read(data)[0])
    for bad in (data.replace(b"32-bit_rle_rgbe", b"32-bit_rle_xyze"), data.replace(b"-Y 1 +X 9", b"+Y 1 +X 9"), data[:-1], data + b"\0", b"P6\n" + data):
        with pytest.raises(rgbe.RgbeError):
            rgbe.read(bad)
