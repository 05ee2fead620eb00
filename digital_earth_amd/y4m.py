"""A YUV4MPEG2 (.y4m) writer for the planar frames of the video output (include/digital_earth_video.h): pure Python, no dependency.

    with Y4MWriter("flyover.y4m", 1920, 1080, fps=(30, 1), format="i420", range="limited", siting="left") as w:
        w.write(frame)          # a frame of Renderer.fetch_video(): Y, Cb and Cr planes one after the other

The stream is one header line

    YUV4MPEG2 W<width> H<height> F<num>:<den> Ip A1:1 C<420mpeg2|420jpeg|420paldv|420p10> XCOLORRANGE=<LIMITED|FULL>

and, per frame, the line `FRAME` followed by the planes as they are.  Y4M is planar: "i420" (8 bits) and "i010" (10 bits in the low bits of
little-endian words, C420p10) are written; the interleaved "nv12" and "p010" are refused.  The colourspace tag names the chroma siting: 420mpeg2 for
"left", 420jpeg for "center", 420paldv for "topleft" (the nearest tag the format has: chroma co-sited with a luma sample, not between two); 10 bits has the one tag 420p10 and the
siting travels out of band.  The matrix is not part of the format: name it to the consumer."""

FORMATS = ("i420", "i010")
_TAG8 = {"left": "420mpeg2", "center": "420jpeg", "topleft": "420paldv"}
_RANGE = {"limited": "LIMITED", "full": "FULL"}


def header(width, height, fps=(30, 1), format="i420", range="limited", siting="left"):
    """The stream header line, as bytes, newline included."""
    if format in ("nv12", "p010"):
        raise ValueError("Y4M holds planar frames: set the video output to I420 instead of NV12, or I010 instead of P010 (got %r)" % (format,))
    if format not in FORMATS:
        raise ValueError("format must be one of %s" % (FORMATS,))
    if range not in _RANGE:
        raise ValueError("range must be 'limited' or 'full'")
    if siting not in _TAG8:
        raise ValueError("siting must be 'left', 'center' or 'topleft'")
    width, height = int(width), int(height)
    if width <= 0 or height <= 0 or width % 2 or height % 2:
        raise ValueError("a 4:2:0 frame has a positive even width and height (got %d x %d)" % (width, height))
    num, den = (int(fps[0]), int(fps[1])) if isinstance(fps, (tuple, list)) else (int(fps), 1)
    if num <= 0 or den <= 0:
        raise ValueError("fps must be a positive ratio")
    tag = "420p10" if format == "i010" else _TAG8[siting]
    return ("YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C%s XCOLORRANGE=%s\n" % (width, height, num, den, tag, _RANGE[range])).encode("ascii")


def frame_bytes(width, height, format="i420"):
    return int(width) * int(height) * 3 // 2 * (2 if format == "i010" else 1)


class Y4MWriter:
    def __init__(self, path, width, height, fps=(30, 1), format="i420", range="limited", siting="left"):
        self._head = header(width, height, fps, format, range, siting)      # raises before the file is created
        self.width, self.height, self.format = int(width), int(height), format
        self.frame_bytes = frame_bytes(width, height, format)
        self.frames = 0
        self._f = open(path, "wb")
        self._f.write(self._head)

    def write(self, frame):
        """One frame: anything with the buffer interface (bytes, a numpy array of any shape) holding exactly frame_bytes bytes, planes Y, Cb, Cr."""
        data = memoryview(frame)
        if not data.c_contiguous:
            raise ValueError("the frame must be contiguous")
        if data.nbytes != self.frame_bytes:
            raise ValueError("the frame holds %d bytes, %d x %d %s takes %d" % (data.nbytes, self.width, self.height, self.format, self.frame_bytes))
        self._f.write(b"FRAME\n")
        self._f.write(data.cast("B") if data.format != "B" or data.ndim != 1 else data)
        self.frames += 1

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def read(path):
    """Parse a file this module wrote: (tokens, frames) — the header's tokens as a list of str and the frames as a list of bytes.  For tests and small files."""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"\n")
    tokens = blob[:end].decode("ascii").split(" ")
    if tokens[0] != "YUV4MPEG2":
        raise ValueError("not a YUV4MPEG2 stream")
    w = int([t for t in tokens if t[0] == "W"][0][1:])
    h = int([t for t in tokens if t[0] == "H"][0][1:])
    tag = [t for t in tokens if t[0] == "C"][0][1:]
    n = w * h * 3 // 2 * (2 if tag == "420p10" else 1)
    frames, at = [], end + 1
    while at < len(blob):
        if blob[at:at + 6] != b"FRAME\n":
            raise ValueError("no FRAME marker at byte %d" % at)
        frames.append(blob[at + 6:at + 6 + n])
        if len(frames[-1]) != n:
            raise ValueError("a short frame")
        at += 6 + n
    return tokens, frames
