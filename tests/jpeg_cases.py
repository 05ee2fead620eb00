"""The sizes and inputs the JPEG output is held to (tests/test_jpeg_ref.py on the CPU, tests/test_gpu_jpeg.py on the GPU), each input with the
precondition that makes it reach its branch, asserted on the reference stream.  Images and reference streams are built once and never written to."""
import functools

import numpy as np

import jpeg_ref as jr

F = np.float32
# (W, H, restart): one MCU; all padding; ragged on both axes; H = 8 mod 16; ten intervals (RST7 wraps to RST0); restart 1, 3 (does not divide 8), one interval
SIZES = [(16, 16, 8), (2, 2, 8), (34, 18, 8), (48, 40, 8), (160, 16, 1), (64, 32, 1), (64, 32, 3), (64, 32, 65535)]
QUALITY = dict(black=100, white=100, checker77=50, impulse=100, noise100=100, noise1=1, specials=90)
INPUTS = tuple(QUALITY)
# Frames of more than 1024 restart intervals, where a thread of jpeg_scan_kernel owns more than one: a list of their own, so that the full input set does
# not run at these sizes.  528 x 528 is 33 x 33 MCUs: two intervals per thread, the last owner has one and 479 threads none; 544 x 1040 is 34 x 65: three
# per thread, the last owner has two.  noise100 gives every interval another length, so a wrong offset shows; black gives every interval the same.
LARGE_SIZES = [(528, 528, 1), (544, 1040, 1)]
LARGE_INPUTS = ("noise100", "black")
SCAN_THREADS = 1024             # JP_SCAN_THREADS of csrc/jpeg_kernels.hip


def scan_geometry(intervals):
    """jpeg_scan_kernel's split of the intervals over its one workgroup, restated from jp_scan_chunk: (intervals per owning thread, owning threads,
    threads that own none, intervals of the last owner)."""
    chunk = -(-intervals // SCAN_THREADS)
    owners = -(-intervals // chunk)
    return chunk, owners, SCAN_THREADS - owners, intervals - (owners - 1) * chunk


def _basis7(n):
    return np.cos((2 * (np.arange(n) % 8) + 1) * 7 * np.pi / 16.0)


@functools.lru_cache(maxsize=None)
def image(name, W, H):
    """(W, H, 3) float32, image[u, v] with v = 0 at the bottom; picture row r is v = H - 1 - r."""
    rng = np.random.default_rng(1000 * W + H)
    if name == "black":
        img = np.zeros((W, H, 3), F)
    elif name == "white":
        img = np.ones((W, H, 3), F)
    elif name == "checker77":       # every 8 x 8 block of the picture is the (7, 7) basis function: grey, so the chroma planes are flat
        r = np.arange(H)[::-1]      # the picture row of image row v
        t = 0.5 + 0.45 * np.outer(_basis7(W), np.cos((2 * (r % 8) + 1) * 7 * np.pi / 16.0)) / np.cos(np.pi / 16.0) ** 2
        img = np.repeat(t[:, :, None], 3, axis=2).astype(F)
    elif name == "impulse":         # one white pixel in the top-left corner of the picture, on black
        img = np.zeros((W, H, 3), F)
        img[0, H - 1] = 1.0
    elif name in ("noise100", "noise1"):
        img = rng.uniform(0.0, 1.0, (W, H, 3)).astype(F)
    elif name == "specials":
        img = rng.uniform(0.0, 1.0, (W, H, 3)).astype(F)
        flat = img.reshape(-1)
        flat[0::7] = np.nan
        flat[1::7] = -0.0
        flat[2::7] = np.inf
    else:
        raise KeyError(name)
    img.flags.writeable = False
    return img


@functools.lru_cache(maxsize=None)
def reference(name, W, H, restart):
    """(the reference's file, its statistics, its coefficients)."""
    stats = {}
    data = jr.encode(image(name, W, H), QUALITY[name], restart, stats)
    q, _, _ = jr.coefficients(image(name, W, H), QUALITY[name])
    return data, stats, q


def check_precondition(name, W, H, restart):
    """The case reaches the branch it is there for — so that it cannot pass empty."""
    data, st, q = reference(name, W, H, restart)
    mcus = q.shape[0]
    scan = data[jr.FRAMING_BYTES:-2]
    assert st["intervals"] == -(-mcus // min(restart, mcus))
    if name in ("black", "white"):
        assert st["eob_only"] == 6 * mcus                                    # EOB-only blocks
        assert st["max_dc_category"] == (11 if name == "black" else 10)      # DC saturation: -1024 and 1016 at Q = 1
        assert int(q[0, 0, 0]) == (-1024 if name == "black" else 1016)
    elif name == "checker77":
        luma = q[:, :4]
        single = ((luma[..., 63] != 0) & (luma[..., :63] == 0).all(axis=-1)).sum()      # blocks of a single, last coefficient:
        inside = (W // 8) * (H // 8)                                          # every luminance block that lies inside the picture (2 x 2 has none)
        assert single >= inside and (single == 4 * mcus or W % 16 or H % 16)
        assert st["zrl"] >= 3 * inside and (st["last_position"] == 63 or not inside)      # three ZRLs in front of it, no EOB behind it
        assert (q[:, 4:, 1:] == 0).all()
    elif name == "impulse":
        assert (q[0, 0, 1:] != 0).all()                                       # every AC position of the first block
    elif name == "noise100":
        assert b"\xff\x00" in scan or W * H <= 4, "no stuffed byte"           # (the 2 x 2 frame is one flat MCU: too short to promise one)
        assert st["longest_ac_code"] == 16 or W * H <= 4
    elif name == "noise1":
        Qy, Qc = jr.quant_tables(1)
        assert (Qy == 255).all() and (Qc == 255).all()                        # Q clamps to 255
        assert (q[..., 1:] == 0).mean() > 0.75                                # blocks of mostly zeros
    elif name == "specials":
        img = image(name, W, H)
        clean = np.where(np.isnan(img), F(0), np.where(np.isinf(img), F(1), img)).astype(F)
        assert np.isnan(img).any() and np.isinf(img).any() and (np.signbit(img) & (img == 0)).any()
        assert jr.encode(clean, QUALITY[name], restart) == data               # the inherited clamp: NaN and -0.0 are 0, +inf is 1
    if (W, H, restart) == (160, 16, 1):
        assert st["intervals"] == 10 and bytes([0xff, 0xd7]) in data and data.count(bytes([0xff, 0xd0])) >= 2      # RST7 wraps to RST0
