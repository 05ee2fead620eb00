"""An independent reading of a baseline JPEG file (ITU-T T.81) in plain Python / numpy, and the float64 DCT of tests/jpeg_ref.py's blocks: no code shared
with the encoder side of jpeg_ref.py.  decode() reads the markers, builds the Huffman tables from the stream's OWN DHT segments, undoes the byte stuffing
and the restart markers, and returns the quantised coefficients and the tables as the file states them."""
import numpy as np


def _huffman_lookup(bits, vals):
    """{(length, code): symbol} from BITS and HUFFVAL (Annex C)."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


class _Reader:
    def __init__(self, data):
        self.bits = "".join(format(b, "08b") for b in data)
        self.at = 0

    def take(self, n):
        v = int(self.bits[self.at:self.at + n], 2) if n else 0
        assert self.at + n <= len(self.bits), "the scan ran out of bits"
        self.at += n
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.take(1)
            if (length, code) in table:
                return table[(length, code)]
        raise AssertionError("no Huffman code of 16 bits or fewer matches")

    def value(self, n):
        if not n:
            return 0
        v = self.take(n)
        return v if v >> (n - 1) else v - (1 << n) + 1


def decode(data):
    """A dict: width, height, components [(id, h, v, tq)], qtables {id: int array [64] in NATURAL order}, restart, markers (the sequence of marker
    bytes in front of the scan), intervals (the number of restart intervals), rst (the RSTm numbers met), and coef: int32 [mcus][blocks per MCU][64] in
    zigzag order, blocks in scan order."""
    data = bytes(data)
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    zz = _zigzag()
    out = dict(qtables={}, markers=[0xd8], restart=0, app0=None)
    huff = {}
    at = 2
    while True:
        assert data[at] == 0xff
        marker = data[at + 1]
        n = int.from_bytes(data[at + 2:at + 4], "big")
        body = data[at + 4:at + 2 + n]
        out["markers"].append(marker)
        if marker == 0xe0:
            out["app0"] = body
        elif marker == 0xdb:
            k = 0
            while k < len(body):
                assert body[k] >> 4 == 0, "8-bit precision"
                q = np.zeros(64, dtype=np.int32)
                q[zz] = list(body[k + 1:k + 65])
                out["qtables"][body[k] & 15] = q
                k += 65
        elif marker == 0xc0:
            assert body[0] == 8
            out["height"], out["width"] = int.from_bytes(body[1:3], "big"), int.from_bytes(body[3:5], "big")
            out["components"] = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])]
        elif marker == 0xc4:
            k = 0
            while k < len(body):
                bits = list(body[k + 1:k + 17])
                m = sum(bits)
                huff[(body[k] >> 4, body[k] & 15)] = _huffman_lookup(bits, list(body[k + 17:k + 17 + m]))
                k += 17 + m
        elif marker == 0xdd:
            out["restart"] = int.from_bytes(body, "big")
        elif marker == 0xda:
            ns = body[0]
            scan = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(ns)]
            assert tuple(body[1 + 2 * ns:4 + 2 * ns]) == (0, 63, 0)
            at += 2 + n
            break
        else:
            raise AssertionError("unexpected marker %02x" % marker)
        at += 2 + n
    # the entropy-coded segments: split at markers, unstuff
    segments, cur, rst = [], bytearray(), []
    k = at
    while True:
        b = data[k]
        if b == 0xff:
            nxt = data[k + 1]
            if nxt == 0x00:
                cur.append(0xff)
                k += 2
                continue
            segments.append(bytes(cur))
            cur = bytearray()
            if nxt == 0xd9:
                assert k + 2 == len(data)
                break
            assert 0xd0 <= nxt <= 0xd7, "marker %02x inside the scan" % nxt
            rst.append(nxt - 0xd0)
            k += 2
            continue
        cur.append(b)
        k += 1
    comps = {cid: (h, v, tq) for cid, h, v, tq in out["components"]}
    hmax, vmax = max(h for h, _, _ in comps.values()), max(v for _, v, _ in comps.values())
    mcus = -(-out["width"] // (8 * hmax)) * -(-out["height"] // (8 * vmax))
    per = out["restart"] if out["restart"] else mcus
    assert len(segments) == -(-mcus // per), (len(segments), mcus, per)
    order = [(cid, td, ta) for cid, td, ta in scan for _ in range(comps[cid][0] * comps[cid][1])]
    coef = np.zeros((mcus, len(order), 64), dtype=np.int32)
    m = 0
    for seg in segments:
        r = _Reader(seg)
        pred = {cid: 0 for cid in comps}
        for _ in range(min(per, mcus - m)):
            for j, (cid, td, ta) in enumerate(order):
                pred[cid] += r.value(r.symbol(huff[(0, td)]))
                coef[m, j, 0] = pred[cid]
                pos = 1
                while pos < 64:
                    rs = r.symbol(huff[(1, ta)])
                    if rs == 0x00:
                        break
                    if rs == 0xF0:
                        pos += 16
                        continue
                    pos += rs >> 4
                    coef[m, j, pos] = r.value(rs & 15)
                    pos += 1
                assert pos <= 64
            m += 1
        tail = r.bits[r.at:]
        assert len(tail) < 8 and set(tail) <= {"1"}, "an interval is padded to a byte boundary with 1-bits"
    assert m == mcus
    out.update(coef=coef, intervals=len(segments), rst=rst)
    return out


def _zigzag():
    """Zigzag position -> natural index, walked along the anti-diagonals (T.81 Figure 5) rather than copied from a table."""
    order = []
    for d in range(15):
        cells = [(v, d - v) for v in range(8) if 0 <= d - v < 8]
        order += [v * 8 + u for v, u in (cells if d % 2 else cells[::-1])]
    return np.array(order)


def dct_f64(s):
    """The true 2-D DCT of samples s[..., y, x] in float64: F[..., v, u] = 1/4 c(u) c(v) sum s cos cos."""
    k, x = np.arange(8)[:, None], np.arange(8)[None, :]
    A = 0.5 * np.where(k == 0, np.sqrt(0.5), 1.0) * np.cos((2 * x + 1) * k * np.pi / 16.0)
    return np.einsum("vy,...yx,ux->...vu", A, np.asarray(s, dtype=np.float64), A)


def idct_f64(F):
    k, x = np.arange(8)[:, None], np.arange(8)[None, :]
    A = 0.5 * np.where(k == 0, np.sqrt(0.5), 1.0) * np.cos((2 * x + 1) * k * np.pi / 16.0)
    return np.einsum("vy,...vu,ux->...yx", A, np.asarray(F, dtype=np.float64), A)
