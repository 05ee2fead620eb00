"""Motion-JPEG writers for the files of the JPEG output (include/digital_earth_jpeg.h): pure Python, no dependency.

    with AVIWriter("flyover.avi", 1920, 1080, fps=(30, 1)) as w:
        w.write(jpeg_bytes)           # one complete JPEG file per frame: Renderer.fetch_jpeg()

AVIWriter writes an AVI 1.0 RIFF file every player opens:
    RIFF 'AVI '
      LIST 'hdrl'   avih (56 bytes)
        LIST 'strl' strh (56 bytes: 'vids', 'MJPG', scale / rate = the frame period)   strf (BITMAPINFOHEADER, 40 bytes: 24 bits, 'MJPG')
      LIST 'movi'   one '00dc' chunk per frame, its data padded to an even length (the chunk's size field is the unpadded length)
      idx1          16 bytes per frame: '00dc', AVIIF_KEYFRAME, the chunk's offset from the 'movi' fourcc, its length
The sizes (RIFF, movi) and the frame counts (avih, strh) are patched on close().  An AVI 1.0 file holds less than 2^32 bytes: a frame that would take
the file past that is refused (ValueError) and the file stays valid.  MJPEGWriter writes the frames one after the other with nothing between them
(`.mjpeg`, what `ffmpeg -f mjpeg` reads)."""
import struct

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
LIMIT = 1 << 32


def _is_jpeg(frame):
    return len(frame) >= 4 and bytes(frame[:2]) == b"\xff\xd8" and bytes(frame[-2:]) == b"\xff\xd9"


class MJPEGWriter:
    def __init__(self, path):
        self._f = open(path, "wb")
        self.frames = 0

    def write(self, frame):
        if not _is_jpeg(frame):
            raise ValueError("a frame must be one complete JPEG file (SOI ... EOI)")
        self._f.write(frame)
        self.frames += 1

    def close(self):
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class AVIWriter:
    def __init__(self, path, width, height, fps=(30, 1)):
        self.width, self.height = int(width), int(height)
        self.rate, self.scale = int(fps[0]), int(fps[1])
        if self.width <= 0 or self.height <= 0 or self.rate <= 0 or self.scale <= 0:
            raise ValueError("width, height and both terms of fps must be positive")
        self.frames = 0
        self._index = []            # (offset from the 'movi' fourcc, length) per frame
        self._largest = 0
        self._f = open(path, "wb")
        self._f.write(self._headers())
        self._movi = self._f.tell() - 4       # where the 'movi' fourcc stands
        self._at = self._f.tell()             # the file's length so far

    def _headers(self):
        """Everything in front of the first frame, with the counts and sizes as they stand."""
        n, w, h = self.frames, self.width, self.height
        movi_bytes = 4 + sum(8 + length + (length & 1) for _, length in self._index)
        avih = struct.pack("<14I", self.scale * 1000000 // self.rate, 0, 0, AVIF_HASINDEX, n, 0, 1, self._largest, w, h, 0, 0, 0, 0)
        strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIIIhhhh", 0, 0, 0, 0, self.scale, self.rate, 0, n, self._largest, 0xffffffff, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        head = b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", movi_bytes) + b"movi"
        riff_bytes = len(head) + (movi_bytes - 4) + 8 + 16 * n
        return b"RIFF" + struct.pack("<I", riff_bytes) + head

    def write(self, frame):
        if self._f is None:
            raise ValueError("the writer is closed")
        if not _is_jpeg(frame):
            raise ValueError("a frame must be one complete JPEG file (SOI ... EOI)")
        length = len(frame)
        padded = length + (length & 1)
        if self._at + 8 + padded + 8 + 16 * (self.frames + 1) >= LIMIT:
            raise ValueError("an AVI file holds less than 2^32 bytes: this frame does not fit")
        self._f.write(b"00dc" + struct.pack("<I", length))
        self._f.write(frame)
        if length & 1:
            self._f.write(b"\0")
        self._index.append((self._at - self._movi, length))
        self._at += 8 + padded
        self._largest = max(self._largest, length)
        self.frames += 1

    def close(self):
        if self._f is None:
            return
        self._f.write(b"idx1" + struct.pack("<I", 16 * self.frames))
        for offset, length in self._index:
            self._f.write(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, offset, length))
        self._f.seek(0)
        self._f.write(self._headers())      # the same bytes with the final counts and sizes
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
