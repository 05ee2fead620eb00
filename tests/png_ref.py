"""The PNG output restated in numpy integers (include/digital_earth_png.h is the contract): filter, chunks, tokens, code lengths, the
dynamic / stored decision, alignment, zlib and PNG framing — encode() gives the bytes the GPU must give — and a small, independent decoder: a PNG
parser that checks every CRC with zlib.crc32, inflates with zlib.decompress (which checks the Adler-32) and unfilters."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
TRAILER_BYTES = 28
CHUNK_OVERHEAD = 24
HEADER_BITS = 1222
DEFAULT_CHUNK = 32768
FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")
LEN_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258])
LEN_EXTRA = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0])
LEN_CODE = np.searchsorted(LEN_BASE, np.arange(3, 259), side="right") - 1      # match length - 3 -> index of its code


def _chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def as_rows(px):
    """(H, W, C) uint8 or (H, W, 3) uint16 -> ((H, W * bpp) uint8 as PNG orders the bytes, bpp, depth, colour type)."""
    px = np.asarray(px)
    if px.dtype == np.uint8 and px.ndim == 3 and px.shape[2] in (3, 4):
        return np.ascontiguousarray(px).reshape(px.shape[0], -1), px.shape[2], 8, 2 if px.shape[2] == 3 else 6
    if px.dtype == np.uint16 and px.ndim == 3 and px.shape[2] == 3:
        return px.astype(">u2").view(np.uint8).reshape(px.shape[0], -1), 6, 16, 2
    raise ValueError("pixels must be (H, W, 3 | 4) uint8 or (H, W, 3) uint16")


# ---- the filter
def _candidates(rows, bpp):
    x = rows.astype(np.int32)
    a = np.zeros_like(x); a[:, bpp:] = x[:, :-bpp] if x.shape[1] > bpp else 0
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, bpp:] = x[:-1, :-bpp] if x.shape[1] > bpp else 0
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]) & 255      # (5, H, R)


def filter_rows(rows, bpp, filter="adaptive"):
    """The filtered stream S as (H, 1 + R) uint8 and the row types."""
    cand = _candidates(rows, bpp)
    if filter == "adaptive" or filter == 5:
        cost = np.where(cand < 128, cand, 256 - cand).sum(axis=2)      # (5, H)
        types = np.argmin(cost, axis=0)                                # the first minimum: ties to the lowest type
    else:
        types = np.full(rows.shape[0], FILTERS.index(filter) if isinstance(filter, str) else int(filter))
    S = np.empty((rows.shape[0], 1 + rows.shape[1]), np.uint8)
    S[:, 0] = types
    S[:, 1:] = cand[types, np.arange(rows.shape[0])]
    return S, types


def filter_rows_naive(rows, bpp):
    """The adaptive filter once more as a per-byte loop, written apart from the vectorised one."""
    H, R = rows.shape
    out = []
    prev = [0] * R
    for y in range(H):
        cur = [int(v) for v in rows[y]]
        best = None
        for f in range(5):
            line, cost = [], 0
            for i in range(R):
                left = cur[i - bpp] if i >= bpp else 0
                up = prev[i]
                ul = prev[i - bpp] if i >= bpp else 0
                if f == 0:
                    pred = 0
                elif f == 1:
                    pred = left
                elif f == 2:
                    pred = up
                elif f == 3:
                    pred = (left + up) // 2
                else:
                    p = left + up - ul
                    d = (abs(p - left), abs(p - up), abs(p - ul))
                    pred = left if d[0] <= d[1] and d[0] <= d[2] else (up if d[1] <= d[2] else ul)
                v = (cur[i] - pred) % 256
                line.append(v)
                cost += v if v < 128 else 256 - v
            if best is None or cost < best[0]:
                best = (cost, f, line)
        out.append([best[1]] + best[2])
        prev = cur
    return np.array(out, np.uint8)


# ---- tokens
def tokens(chunk):
    """The chunk's tokens in order as two arrays: (value, length) — length 0 is the literal `value`, otherwise a match of that length, distance 1."""
    c = np.asarray(chunk, np.uint8).astype(np.int64)
    n = len(c)
    i = np.arange(n)
    starts = np.flatnonzero(np.concatenate(([True], c[1:] != c[:-1])))
    run = np.cumsum(np.concatenate(([True], c[1:] != c[:-1]))) - 1
    h = starts[run]
    r = (np.diff(np.concatenate((starts, [n]))) - 1)[run]      # equal bytes behind the run's head
    off = i - h
    k = off - 1
    full, rem = r // 258, r % 258
    q, kk = k // 258, k % 258
    lit = (off == 0) | ((off > 0) & (q == full) & (rem < 3))
    match = (off > 0) & (kk == 0) & ((q < full) | (rem >= 3))
    length = np.where(match, np.where(q < full, 258, rem), 0)
    keep = lit | match
    return c[keep], length[keep]


def expand(values, lengths):
    """Tokens back to bytes, as an inflater would: a match of distance 1 repeats the last byte."""
    out = []
    for v, L in zip(values, lengths):
        if L == 0:
            out.append(int(v))
        else:
            out.extend([out[-1]] * int(L))
    return bytes(out)


# ---- code lengths
def code_lengths(freq):
    """Lengths (<= 15, complete) of the symbols with freq > 0: Moffat-Katajainen on the counts sorted by (count, symbol), the Kraft repair, the hand-out."""
    freq = [int(f) for f in freq]
    order = sorted((s for s in range(len(freq)) if freq[s] > 0), key=lambda s: (freq[s], s))
    m = len(order)
    assert m >= 2
    A = [freq[s] for s in order]
    A[0] += A[1]
    root, leaf = 0, 2
    for nxt in range(1, m - 1):
        if leaf >= m or A[root] < A[leaf]:
            A[nxt] = A[root]; A[root] = nxt; root += 1
        else:
            A[nxt] = A[leaf]; leaf += 1
        if leaf >= m or (root < nxt and A[root] < A[leaf]):
            A[nxt] += A[root]; A[root] = nxt; root += 1
        else:
            A[nxt] += A[leaf]; leaf += 1
    A[m - 2] = 0
    for nxt in range(m - 3, -1, -1):
        A[nxt] = A[A[nxt]] + 1
    avbl, used, depth, root, nxt = 1, 0, 0, m - 2, m - 1
    while avbl > 0:
        while root >= 0 and A[root] == depth:
            used += 1; root -= 1
        while avbl > used:
            A[nxt] = depth; nxt -= 1; avbl -= 1
        avbl, depth, used = 2 * used, depth + 1, 0
    count = [0] * 16
    for l in A:
        count[min(l, 15)] += 1
    total = sum(count[l] << (15 - l) for l in range(1, 16))
    while total != 1 << 15:
        count[15] -= 1
        for l in range(14, 0, -1):
            if count[l]:
                count[l] -= 1; count[l + 1] += 2
                break
        total -= 1
    lengths = [0] * len(freq)
    j = m
    for l in range(1, 16):
        for _ in range(count[l]):
            j -= 1
            lengths[order[j]] = l
    return lengths


def canonical_codes(lengths):
    """RFC 1951 §3.2.2; each code bit-reversed, ready to be packed LSB first."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            codes[s] = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
    return codes


def _pack(values, nbits, total_bits):
    """Fields of `nbits` bits each, LSB first, one behind the other: the bytes (zero-padded)."""
    values, nbits = np.asarray(values, np.int64), np.asarray(nbits, np.int64)
    start = np.concatenate(([0], np.cumsum(nbits)))[:-1]
    bits = np.zeros((total_bits + 7) // 8 * 8, np.uint8)
    for j in range(int(nbits.max()) if len(nbits) else 0):
        m = nbits > j
        bits[start[m] + j] = (values[m] >> j) & 1
    return np.packbits(bits, bitorder="little").tobytes()


def deflate_chunk(chunk, first, final, info=None):
    """The deflate data of one chunk: CMF / FLG in front of the first, the block (dynamic, or stored if that is not longer), the empty stored block
    behind every chunk but the last."""
    chunk = np.asarray(chunk, np.uint8)
    n = len(chunk)
    values, lengths = tokens(chunk)
    is_match = lengths > 0
    idx = LEN_CODE[np.where(is_match, lengths, 3) - 3]
    sym = np.where(is_match, 257 + idx, values)
    freq = np.bincount(sym, minlength=286)
    freq[256] += 1
    ll = code_lengths(freq)
    codes = canonical_codes(ll)
    ll_a, codes_a = np.array(ll), np.array(codes)
    extra = np.where(is_match, LEN_EXTRA[idx], 0)
    tok_bits = ll_a[sym] + extra + is_match      # a match's distance: the single bit 0
    tok_val = codes_a[sym] | (np.where(is_match, lengths - LEN_BASE[idx], 0) << ll_a[sym])
    dyn_bits = HEADER_BITS + int(tok_bits.sum()) + ll[256]
    stored = (dyn_bits + 7) // 8 >= n + 5
    if info is not None:
        info.append("stored" if stored else "dynamic")
    if stored:
        body = bytes([1 if final else 0]) + struct.pack("<HH", n, n ^ 0xffff) + chunk.tobytes()
        end_bit = 8 * len(body)
    else:
        rev4 = lambda v: int(format(v, "04b")[::-1], 2)
        head_v = [1 if final else 0, 2, 29, 0, 15] + [0, 0, 0] + [4] * 16 + [rev4(l) for l in ll] + [rev4(1 if is_match.any() else 0)]
        head_n = [1, 2, 5, 5, 4] + [3] * 19 + [4] * 287
        v = np.concatenate((head_v, tok_val, [codes[256]]))
        b = np.concatenate((head_n, tok_bits, [ll[256]]))
        assert int(b.sum()) == dyn_bits
        body = _pack(v, b, dyn_bits)
        end_bit = dyn_bits
    if not final:
        body = body + b"\x00" * ((end_bit + 3 + 7) // 8 - len(body)) + b"\x00\x00\xff\xff"
    return (b"\x78\x01" if first else b"") + body


# ---- the file
def front(W, H, channels, depth, cicp=(1, 8, 0, 1)):
    out = SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, 6 if channels == 4 else 2, 0, 0, 0))
    if depth == 16:
        out += _chunk(b"cICP", struct.pack("BBBB", *cicp))
    return out


def capacity(W, H, channels, depth, chunk_bytes=DEFAULT_CHUNK):
    N = H * (1 + W * channels * depth // 8)
    return (49 if depth == 16 else 33) + N + CHUNK_OVERHEAD * ((N + chunk_bytes - 1) // chunk_bytes) + TRAILER_BYTES


def encode(px, filter="adaptive", chunk_bytes=DEFAULT_CHUNK, cicp=(1, 8, 0, 1), info=None):
    """The file the GPU writes for these packed pixels.  info: a list that receives "stored" / "dynamic" per chunk."""
    rows, bpp, depth, _ = as_rows(px)
    H, W = px.shape[:2]
    S = filter_rows(rows, bpp, filter)[0].reshape(-1)
    N = len(S)
    cuts = list(range(0, N, chunk_bytes))
    out = [front(W, H, px.shape[2], depth, cicp)]
    for k, lo in enumerate(cuts):
        out.append(_chunk(b"IDAT", deflate_chunk(S[lo:lo + chunk_bytes], k == 0, k == len(cuts) - 1, info)))
    out.append(_chunk(b"IDAT", struct.pack(">I", zlib.adler32(S.tobytes()) & 0xffffffff)))
    out.append(_chunk(b"IEND", b""))
    return b"".join(out)


def filtered_stream(px, filter="adaptive"):
    rows, bpp, _, _ = as_rows(px)
    return filter_rows(rows, bpp, filter)[0].reshape(-1)


def decode(data):
    """A PNG file -> (pixels (H, W, C) uint8 or uint16, {"cicp": bytes or None, "idats": n}).  Every chunk's CRC, IHDR and the zlib stream are checked."""
    data = bytes(data)
    assert data[:8] == SIGNATURE, "not a PNG signature"
    at, idat, ihdr, cicp, idats, ended = 8, [], None, None, 0, False
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert len(body) == n and struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body) & 0xffffffff, "bad CRC in %r" % kind
        at += 12 + n
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"cICP":
            assert not idat
            cicp = body
        elif kind == b"IDAT":
            idat.append(body); idats += 1
        elif kind == b"IEND":
            ended = True
            break
    assert ended and at == len(data), "no IEND at the end of the file"
    W, H, depth, ctype, comp, flt, lace = ihdr
    assert depth in (8, 16) and ctype in (2, 6) and (comp, flt, lace) == (0, 0, 0)
    bpp = (3 if ctype == 2 else 4) * depth // 8
    R = W * bpp
    S = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    assert len(S) == H * (1 + R)
    S = S.reshape(H, 1 + R)
    rows = np.zeros((H, R), np.int32)
    prev = np.zeros(R, np.int32)
    for y in range(H):
        f, line = int(S[y, 0]), S[y, 1:].astype(np.int32)
        assert f <= 4
        cur = np.zeros(R, np.int32)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        else:
            for i in range(R):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                if f == 1:
                    pred = a
                elif f == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[i] = (line[i] + pred) & 255
        rows[y] = cur
        prev = cur
    raw = rows.astype(np.uint8)
    px = raw.reshape(H, W, bpp) if depth == 8 else raw.reshape(H, W, 3, 2).copy().view(">u2").reshape(H, W, 3).astype(np.uint16)
    return px, {"cicp": cicp, "idats": idats}
