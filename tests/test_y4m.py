"""The Y4M writer (digital_earth_amd/y4m.py) without a GPU: frames written from arrays come back byte for byte from a parse of the file, the header holds
the tokens a player needs, and what Y4M cannot hold is refused before a file exists."""
import os

import numpy as np
import pytest

import video_ref as vr
from digital_earth_amd import y4m


def _image(W, H, seed):
    return np.random.default_rng(seed).uniform(0, 1, (W, H, 3)).astype(np.float32)


@pytest.mark.parametrize("format,siting,range_,tag", (("i420", "left", "limited", "C420mpeg2"), ("i420", "center", "full", "C420jpeg"),
                                                      ("i420", "topleft", "limited", "C420paldv"), ("i010", "topleft", "limited", "C420p10"),
                                                      ("i010", "left", "full", "C420p10")))
def test_frames_round_trip(tmp_path, format, siting, range_, tag):
    W, H = 18, 10
    frames = [vr.pack(_image(W, H, k), format, "bt709", range_, siting) for k in range(3)]
    path = str(tmp_path / "a.y4m")
    with y4m.Y4MWriter(path, W, H, fps=(24000, 1001), format=format, range=range_, siting=siting) as w:
        w.write(frames[0])
        w.write(frames[1].tobytes())                                   # bytes ...
        w.write(frames[2].view("<u2") if format == "i010" else frames[2].reshape(-1, W // 2))      # ... or an array of another shape or item size
        assert w.frames == 3 and w.frame_bytes == frames[0].nbytes
    blob = open(path, "rb").read()
    head = ("YUV4MPEG2 W18 H10 F24000:1001 Ip A1:1 %s XCOLORRANGE=%s\n" % (tag, range_.upper())).encode()
    assert blob.startswith(head) and len(blob) == len(head) + 3 * (6 + frames[0].nbytes)
    tokens, got = y4m.read(path)
    assert tokens == head.decode().strip().split(" ")
    assert len(got) == 3 and all(g == f.tobytes() for g, f in zip(got, frames))
    y, cb, cr = vr.planes(np.frombuffer(got[1], np.uint8), W, H, format)                           # the planes are where a reader looks for them
    want = vr.codes(_image(W, H, 1), format, "bt709", range_, siting)
    assert (y == want[0]).all() and (cb == want[1]).all() and (cr == want[2]).all()


def test_default_header_and_integer_fps():
    assert y4m.header(64, 32) == b"YUV4MPEG2 W64 H32 F30:1 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED\n"
    assert y4m.header(64, 32, fps=25).split(b" ")[3] == b"F25:1"
    assert y4m.frame_bytes(64, 32, "i420") == 64 * 32 * 3 // 2 and y4m.frame_bytes(64, 32, "i010") == 64 * 32 * 3


def test_what_y4m_cannot_hold_is_refused(tmp_path):
    path = str(tmp_path / "no.y4m")
    for format, planar in (("nv12", "I420"), ("p010", "I010")):
        with pytest.raises(ValueError) as e:
            y4m.Y4MWriter(path, 16, 8, format=format)
        assert planar in str(e.value)
    for W, H in ((17, 8), (16, 9), (0, 8), (16, -2)):
        with pytest.raises(ValueError):
            y4m.Y4MWriter(path, W, H)
    for kw in (dict(format="yuv444"), dict(range="video"), dict(siting="right"), dict(fps=(0, 1))):
        with pytest.raises(ValueError):
            y4m.Y4MWriter(path, 16, 8, **kw)
    assert not os.path.exists(path)                                     # refused before the file is created
    with y4m.Y4MWriter(path, 16, 8) as w:
        with pytest.raises(ValueError):
            w.write(np.zeros(16 * 8 * 3 // 2 - 1, np.uint8))            # a short frame
        with pytest.raises(ValueError):
            w.write(np.zeros(16 * 8 * 3, np.uint8))                     # a 10-bit frame into an 8-bit file
        assert w.frames == 0
    assert y4m.read(path)[1] == []
