"""The JPEG output's numpy restatement (tests/jpeg_ref.py) held to an independent reading of ITU-T T.81 without a GPU: an independent decoder
(tests/jpeg_f64.py) gets the reference's coefficients back exactly from every reference stream; every coefficient is the float64 DCT's within half a
step plus a bound derived here from the integer table and the row rounding; Pillow opens every stream; the tables are Annex K's."""
import io

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_f64 as j64
import jpeg_ref as jr

CASES = [(name, W, H, restart) for (W, H, restart) in jc.SIZES for name in jc.INPUTS]
# the frames of more than 1024 intervals (tests/test_gpu_large_geometry.py): the reference is held to the decoder and to Pillow at these sizes too
CASES += [(name, W, H, restart) for (W, H, restart) in jc.LARGE_SIZES for name in jc.LARGE_INPUTS]


def _ids(case):
    return "%s-%dx%d-r%d" % case


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_decoder_returns_the_reference_coefficients(case):
    name, W, H, restart = case
    jc.check_precondition(name, W, H, restart)
    data, st, q = jc.reference(name, W, H, restart)
    d = j64.decode(data)
    assert (d["width"], d["height"], d["restart"]) == (W, H, restart)
    assert d["components"] == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    assert d["markers"] == [0xd8, 0xe0, 0xdb, 0xdb, 0xc0, 0xc4, 0xc4, 0xc4, 0xc4, 0xdd, 0xda]
    assert d["app0"] == b"JFIF\0\x01\x02\x00\x00\x01\x00\x01\x00\x00"
    assert d["intervals"] == st["intervals"] and d["rst"] == [i % 8 for i in range(st["intervals"] - 1)]
    Qy, Qc = jr.quant_tables(jc.QUALITY[name])
    assert (d["qtables"][0] == Qy).all() and (d["qtables"][1] == Qc).all()
    assert d["coef"].shape == q.shape and (d["coef"] == q).all()
    assert len(data) <= jr.capacity(W, H, restart)


def dct_error_bound():
    """b: how far F / 2^18 can lie from the float64 DCT, from the table M and the row rounding alone.  With A the exact matrix (entries 1/2 c cos) and
    M = 2^14 A + e, |e| <= 1/2 per entry (measured on the table itself), |s| <= 128:
      rows     T / 2^14 = A s + e s / 2^14                  error at most   128 sum_x |e[u][x]| / 2^14
      rounding T' = T / 2^10 + r, |r| <= 1/2                error at most   (1/2) / 2^4 in units of A s (T' carries 2^4 A s)
      columns  F / 2^18 = sum_y (A + e / 2^14)[v][y] T'[y][u] / 2^4:  the row errors pass through sum_y |A[v][y]|, and e[v][y] meets |T'| <= 5793."""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    A = 0.5 * np.where(u == 0, np.sqrt(0.5), 1.0) * np.cos((2 * x + 1) * u * np.pi / 16.0)
    e = np.abs(jr.dct_matrix().astype(np.float64) - 16384.0 * A)
    assert e.max() <= 0.5
    row_err = 128.0 * e.sum(axis=1).max() / 16384.0 + 0.5 / 16.0
    tprime_max = (np.abs(jr.dct_matrix()).sum(axis=1).max() * 128 + 512) // 1024
    return float(np.abs(A).sum(axis=1).max() * row_err + e.sum(axis=1).max() * tprime_max / 16384.0 / 16.0)


@pytest.mark.parametrize("name", jc.INPUTS)
def test_every_coefficient_is_the_float64_dct_within_half_a_step(name):
    b = dct_error_bound()
    assert b < 0.5, b
    for W, H, _ in [(34, 18, 8), (64, 32, 1)]:
        q, Qy, Qc = jr.coefficients(jc.image(name, W, H), jc.QUALITY[name])
        F64 = j64.dct_f64(jr.blocks(jc.image(name, W, H))).reshape(q.shape[0], 6, 64)[:, :, jr.ZIGZAG]
        Q = np.stack([Qy[jr.ZIGZAG]] * 4 + [Qc[jr.ZIGZAG]] * 2).astype(np.float64)[None]
        err = np.abs(q - F64 / Q)
        assert (err <= 0.5 + b / Q).all(), (name, W, H, float((err - 0.5 - b / Q).max()))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_pillow_opens_every_reference_stream(case):
    Image = pytest.importorskip("PIL.Image")
    name, W, H, restart = case
    data, _, q = jc.reference(name, W, H, restart)
    im = Image.open(io.BytesIO(data))
    assert im.format == "JPEG" and im.size == (W, H) and len(im.getbands()) == 3
    im.draft("YCbCr", (W, H))
    im.load()
    assert im.mode == "YCbCr"
    y = np.asarray(im)[..., 0].astype(np.int64)
    # the float64 inverse DCT of the decoded coefficients, clamped and rounded: IEEE 1180 allows a conforming IDCT a peak error of 1
    d = j64.decode(data)
    Qy = d["qtables"][0]
    nat = np.zeros((q.shape[0], 4, 64))
    nat[:, :, jr.ZIGZAG] = d["coef"][:, :4] * Qy[jr.ZIGZAG]
    pix = np.clip(np.rint(j64.idct_f64(nat.reshape(-1, 4, 8, 8)) + 128.0), 0, 255)
    mx, my = (W + 15) // 16, (H + 15) // 16
    full = pix.reshape(my, mx, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(my * 16, mx * 16)[:H, :W]
    assert np.abs(y - full).max() <= 1


def test_tables_are_annex_k():
    Qy, Qc = jr.quant_tables(50)
    assert (Qy == jr.K1).all() and (Qc == jr.K2).all() and Qy[0] == 16 and Qy[63] == 99 and Qc[0] == 17
    for Q in jr.quant_tables(100):
        assert (Q == 1).all()
    assert all(len(vals) == sum(bits) for bits, vals in (jr.DC_LUMA, jr.DC_CHROMA, jr.AC_LUMA, jr.AC_CHROMA))
    assert len(jr.AC_LUMA[1]) == len(jr.AC_CHROMA[1]) == 162 and sorted(jr.AC_LUMA[1]) == sorted(jr.AC_CHROMA[1])
    assert (np.sort(jr.ZIGZAG) == np.arange(64)).all() and (jr.ZIGZAG == j64._zigzag()).all()
    M = jr.dct_matrix()
    assert M.dtype == np.int32 and (M[0] == 5793).all() and M[1, 0] == 8035 and M[4, 0] == 5793 and M[4, 1] == -5793


def test_pillow_writes_the_same_typical_tables():
    """Pillow's own encoder (libjpeg) ships Annex K's tables too: its quality-50 DQT and its DHT segments equal the reference's byte for byte."""
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.new("RGB", (16, 16), (10, 200, 90)).save(buf, "JPEG", quality=50, subsampling=2, optimize=False)
    theirs, ours = buf.getvalue(), jr.framing(16, 16, 50, 8)

    def segments(data, marker):
        out, at = [], 2
        while data[at + 1] != 0xda:
            n = int.from_bytes(data[at + 2:at + 4], "big")
            if data[at + 1] == marker:
                out.append(data[at + 4:at + 2 + n])
            at += 2 + n
        return b"".join(out)
    for marker in (0xdb, 0xc4):
        a, b = segments(theirs, marker), segments(ours, marker)
        assert len(a) == len(b) and a == b, hex(marker)
