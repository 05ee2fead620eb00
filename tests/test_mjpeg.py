"""digital_earth_amd/mjpeg.py without a GPU: three tiny frames into an AVI; the RIFF tree is walked in pure Python and every chunk size, every idx1
offset and the frames' bytes are checked; Pillow opens frame 1 cut out of the file."""
import io
import struct

import numpy as np
import pytest

import jpeg_ref as jr
from digital_earth_amd import mjpeg


def _frames():
    rng = np.random.default_rng(5)
    return [jr.encode(rng.uniform(0, 1, (16, 16, 3)).astype(np.float32), q, 1) for q in (90, 35, 100)]      # even and odd lengths among them


def _walk(data, at, end, depth=0, out=None):
    out = [] if out is None else out
    while at < end:
        four, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        if four in (b"RIFF", b"LIST"):
            out.append((depth, four + b":" + data[at + 8:at + 12], at, size))
            _walk(data, at + 12, at + 8 + size, depth + 1, out)
        else:
            out.append((depth, four, at, size))
        at += 8 + size + (size & 1)
    assert at == end, "a chunk overruns its parent"
    return out


def test_avi_tree_index_and_frames(tmp_path):
    frames = _frames()
    assert {len(f) & 1 for f in frames} == {0, 1}
    path = str(tmp_path / "t.avi")
    with mjpeg.AVIWriter(path, 16, 16, fps=(25, 1)) as w:
        for f in frames:
            w.write(memoryview(f))
        with pytest.raises(ValueError):
            w.write(b"not a jpeg")
    assert w.frames == 3
    data = open(path, "rb").read()
    tree = _walk(data, 0, len(data))
    assert [(d, n) for d, n, _, _ in tree] == [(0, b"RIFF:AVI "), (1, b"LIST:hdrl"), (2, b"avih"), (2, b"LIST:strl"), (3, b"strh"), (3, b"strf"),
                                               (1, b"LIST:movi"), (2, b"00dc"), (2, b"00dc"), (2, b"00dc"), (1, b"idx1")]
    by = {n: (at, size) for _, n, at, size in tree if n != b"00dc"}
    assert by[b"RIFF:AVI "] == (0, len(data) - 8)
    assert by[b"avih"][1] == 56 and by[b"strh"][1] == 56 and by[b"strf"][1] == 40 and by[b"idx1"][1] == 48
    avih = struct.unpack("<14I", data[by[b"avih"][0] + 8:by[b"avih"][0] + 64])
    assert avih[0] == 40000 and avih[3] & 0x10 and avih[4] == 3 and avih[6] == 1 and avih[7] == max(map(len, frames)) and avih[8:10] == (16, 16)
    strh = data[by[b"strh"][0] + 8:by[b"strh"][0] + 64]
    assert strh[:8] == b"vidsMJPG" and struct.unpack("<II", strh[20:28]) == (1, 25) and struct.unpack("<I", strh[32:36])[0] == 3
    strf = struct.unpack("<IiiHH4sIiiII", data[by[b"strf"][0] + 8:by[b"strf"][0] + 48])
    assert strf[:6] == (40, 16, 16, 1, 24, b"MJPG")
    movi = by[b"LIST:movi"][0] + 8                                   # where the 'movi' fourcc stands
    chunks = [(at, size) for _, n, at, size in tree if n == b"00dc"]
    idx = data[by[b"idx1"][0] + 8:]
    for k, (at, size) in enumerate(chunks):
        assert size == len(frames[k]) and data[at + 8:at + 8 + size] == frames[k]
        assert struct.unpack("<4sIII", idx[16 * k:16 * k + 16]) == (b"00dc", 0x10, at - movi, size)
        assert (at + 8 + size + (size & 1)) % 2 == 0
    Image = pytest.importorskip("PIL.Image")
    at, size = chunks[1]
    im = Image.open(io.BytesIO(data[at + 8:at + 8 + size]))
    im.load()
    assert im.size == (16, 16)


def test_avi_refuses_what_does_not_fit_and_mjpeg_concatenates(tmp_path, monkeypatch):
    frames = _frames()
    path = str(tmp_path / "small.avi")
    monkeypatch.setattr(mjpeg, "LIMIT", 2200)
    w = mjpeg.AVIWriter(path, 16, 16)
    w.write(frames[0])
    with pytest.raises(ValueError, match="2\\^32"):
        w.write(frames[2])
    w.close()
    data = open(path, "rb").read()
    assert len(data) < 2200 and struct.unpack("<I", data[4:8])[0] == len(data) - 8 and len(_walk(data, 0, len(data))) == 9      # still a valid file of one frame
    with pytest.raises(ValueError):
        mjpeg.AVIWriter(str(tmp_path / "bad.avi"), 0, 16)
    path = str(tmp_path / "t.mjpeg")
    with mjpeg.MJPEGWriter(path) as m:
        for f in frames:
            m.write(f)
    assert m.frames == 3 and open(path, "rb").read() == b"".join(frames)
