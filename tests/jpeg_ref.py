"""The JPEG output (include/digital_earth_jpeg.h) restated in numpy integers on top of tests/video_ref.py's planes: the whole file image,
so that the device's stream can be held to it byte for byte.

    encode(image, quality, restart)      ->  bytes: the complete JFIF file
    coefficients(image, quality)         ->  (q, Qy, Qc): int32 [mcus][6][64] in zigzag order (Y0 Y1 Y2 Y3 Cb Cr per MCU) and the two tables (natural order)
    blocks(image)                        ->  int32 [mcus][6][8][8]: the samples s = code - 128 of every block, edges repeated

image is the display's output: (W, H, 3) float32, image[u, v] with v = 0 at the bottom; W and H even."""
import numpy as np

import video_ref as vr

DEFAULTS = dict(quality=90, restart=None)
DEFAULT_RESTART = 2
FRAMING_BYTES = 629
BLOCK_BITS = 22 + 63 * 26      # the worst case of one block before stuffing (csrc/jpeg_kernels.hip)

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
K1 = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
               18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
K2 = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
# Annex K.3 - K.6 as (BITS, HUFFVAL)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def dct_matrix():
    """M[u][x] = rint(2^14 * 1/2 c(u) cos((2 x + 1) u pi / 16)) in double, as int32."""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    c = np.where(u == 0, np.sqrt(0.5), 1.0)
    return np.rint(16384.0 * 0.5 * c * np.cos((2 * x + 1) * u * np.pi / 16.0)).astype(np.int32)


def quant_tables(quality):
    """The IJG rule in integers: (luminance, chrominance), natural order."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError("quality must lie in 1 ... 100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base.astype(np.int64) * scale + 50) // 100, 1, 255).astype(np.int32) for base in (K1, K2))


def huffman_codes(spec):
    """{symbol: (code, length)} of a (BITS, HUFFVAL) pair (T.81 Annex C)."""
    bits, vals = spec
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def planes(image):
    """JFIF's Y'CbCr of the image: (Y [H][W], Cb [H/2][W/2], Cr) as int32 codes, rows top-down."""
    image = np.asarray(image, dtype=np.float32)
    W, H = image.shape[:2]
    if W <= 0 or H <= 0 or W % 2 or H % 2:
        raise ValueError("a 4:2:0 frame has an even width and height")
    frame = vr.pack(image, "i420", "bt601", "full", "center", "round", 0, 0)
    return tuple(p.astype(np.int32) for p in vr.planes(frame, W, H, "i420"))


def _tiles(plane, n_y, n_x):
    """[n_y][n_x][8][8] blocks of a plane padded by repeating its last row and column."""
    h, w = plane.shape
    rows = np.minimum(np.arange(n_y * 8), h - 1)
    cols = np.minimum(np.arange(n_x * 8), w - 1)
    p = plane[rows][:, cols]
    return p.reshape(n_y, 8, n_x, 8).transpose(0, 2, 1, 3)


def blocks(image):
    y, cb, cr = planes(image)
    H, W = y.shape
    mx, my = (W + 15) // 16, (H + 15) // 16
    ty = _tiles(y, 2 * my, 2 * mx).reshape(my, 2, mx, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(my * mx, 4, 8, 8)      # Y0 Y1 / Y2 Y3 in raster order
    tc = [_tiles(c, my, mx).reshape(my * mx, 1, 8, 8) for c in (cb, cr)]
    return np.concatenate([ty] + tc, axis=1).astype(np.int32) - 128


def forward(s):
    """F[..., v, u] of samples s[..., y, x]: the header's two integer passes, int64 here so that an overflow of int32 would show in the assertions."""
    M = dct_matrix().astype(np.int64)
    T = np.einsum("ux,...yx->...yu", M, s.astype(np.int64))
    assert np.abs(T).max(initial=0) <= 5932032
    Tp = (T + 512) >> 10
    F = np.einsum("vy,...yu->...vu", M, Tp)
    assert np.abs(F).max(initial=0) <= 268470792
    return F


def quantise(F, Q):
    """sign(F) ((|F| + D / 2) / D), D = Q << 18; Q[v][u] broadcasts over the leading axes."""
    D = Q.astype(np.int64) << 18
    return (np.sign(F) * ((np.abs(F) + D // 2) // D)).astype(np.int32)


def coefficients(image, quality=90):
    Qy, Qc = quant_tables(quality)
    F = forward(blocks(image))                                   # [mcus][6][8][8]
    Q = np.stack([Qy] * 4 + [Qc] * 2).reshape(6, 8, 8)
    q = quantise(F, Q[None]).reshape(F.shape[0], 6, 64)
    return q[:, :, ZIGZAG], Qy, Qc


class _Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xff
            self.n -= 8
            self.out.append(byte)
            if byte == 0xff:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _value(w, table, symbol_high, v):
    n = int(abs(v)).bit_length()
    code, length = table[symbol_high | n]
    w.put(code, length)
    if n:
        w.put((v - 1 if v < 0 else v) & ((1 << n) - 1), n)
    return n


def entropy(q, restart, stats=None):
    """The entropy-coded data of coefficients q[mcus][6][64] with RSTm between the intervals, without EOI.  stats: a dict that collects what the tests'
    preconditions ask about (the longest AC code, ZRLs, EOB-only blocks, the largest DC category)."""
    dc = [huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA)]
    ac = [huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA)]
    out = bytearray()
    n_mcu = q.shape[0]
    intervals = [(a, min(a + restart, n_mcu)) for a in range(0, n_mcu, restart)]
    st = dict(longest_ac_code=0, zrl=0, eob_only=0, max_dc_category=0, last_position=0, intervals=len(intervals))
    for i, (a, b) in enumerate(intervals):
        w, pred = _Bits(), [0, 0, 0]
        for m in range(a, b):
            for blk in range(6):
                comp, t = max(blk - 3, 0), 1 if blk >= 4 else 0
                c = [int(x) for x in q[m, blk]]
                st["max_dc_category"] = max(st["max_dc_category"], _value(w, dc[t], 0, c[0] - pred[comp]))
                pred[comp] = c[0]
                nz = [k for k in range(1, 64) if c[k]]
                prev = 0
                for k in nz:
                    run = k - prev - 1
                    prev = k
                    while run >= 16:
                        w.put(*ac[t][0xF0])
                        st["zrl"] += 1
                        run -= 16
                    n = int(abs(c[k])).bit_length()
                    assert 1 <= n <= 10
                    st["longest_ac_code"] = max(st["longest_ac_code"], ac[t][(run << 4) | n][1])
                    _value(w, ac[t], run << 4, c[k])
                if prev != 63:
                    w.put(*ac[t][0x00])
                st["eob_only"] += not nz
                st["last_position"] = max(st["last_position"], prev)
        w.pad()
        assert len(w.out) <= 2 * ((6 * (b - a) * BLOCK_BITS + 7) // 8)
        out += w.out
        if i + 1 < len(intervals):
            out += bytes([0xff, 0xd0 + (i & 7)])
    if stats is not None:
        stats.update(st)
    return bytes(out)


def _segment(marker, payload):
    return bytes([0xff, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def framing(W, H, quality, restart):
    """SOI .. SOS: what the host writes once per set_jpeg."""
    Qy, Qc = quant_tables(quality)
    out = bytes([0xff, 0xd8])
    out += _segment(0xe0, b"JFIF\0" + bytes([1, 2, 0, 0, 1, 0, 1, 0, 0]))
    for i, Q in enumerate((Qy, Qc)):
        out += _segment(0xdb, bytes([i]) + bytes(int(x) for x in Q[ZIGZAG]))
    out += _segment(0xc0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xc4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _segment(0xdd, restart.to_bytes(2, "big"))
    out += _segment(0xda, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == FRAMING_BYTES
    return out


def capacity(W, H, restart):
    """de_jpeg_capacity restated: the framing, every interval at its worst case (rounded up to 16), the markers between them, EOI."""
    mcus = ((W + 15) // 16) * ((H + 15) // 16)
    r = min(restart, mcus, 65535)
    intervals = (mcus + r - 1) // r
    slot = (2 * ((r * 6 * BLOCK_BITS + 7) // 8) + 15) // 16 * 16
    return FRAMING_BYTES + intervals * slot + 2 * (intervals - 1) + 2


def encode(image, quality=90, restart=None, stats=None):
    restart = DEFAULT_RESTART if restart is None else int(restart)
    if not 1 <= restart <= 65535:
        raise ValueError("restart must lie in 1 ... 65535")
    image = np.asarray(image, dtype=np.float32)
    W, H = image.shape[:2]
    q, _, _ = coefficients(image, quality)
    return framing(W, H, quality, restart) + entropy(q, restart, stats) + bytes([0xff, 0xd9])
