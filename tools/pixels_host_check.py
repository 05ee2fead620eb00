"""The pixel packs' source on the HOST under the address and undefined-behaviour sanitizers: builds tools/pixels_host_check.cpp
(a stand-alone program that includes csrc/pixels_kernels.hip and csrc/hdr_pack.h, both over csrc/pack.h, and runs each kernel's two halves one
workgroup at a time), feeds it the inputs of tests/test_gpu_pixels.py::test_kernel_equals_the_restatement_byte_for_byte at the three sizes — RGB8 and
RGBA8 of pixels_pack_kernel, RGB10A2 and RGB16 of hdr_pack_kernel, the three modes, the three phases — and compares what it writes with the numpy
restatements (tests/pixels_ref.py, tests/hdr_output_ref.py) byte for byte.  Needs a C++ compiler and no GPU.

    python tools/pixels_host_check.py [--cxx g++] [--keep DIR]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "g++"))
    ap.add_argument("--keep", metavar="DIR")
    args = ap.parse_args()
    import hdr_output_ref as ho
    import pixels_ref as px
    import test_gpu_pixels as t
    work = args.keep or tempfile.mkdtemp(prefix="pixels_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "pixels_host_check")
    subprocess.check_call([args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-x", "c++", os.path.join(ROOT, "tools", "pixels_host_check.cpp"), "-o", exe])
    # the program's format word -> the shape and type of what it writes, and the restatement
    formats = {3: ((3,), np.uint8, lambda img, mode, seed, phase: px.pack(img, 3, mode, seed, phase)),
               4: ((4,), np.uint8, lambda img, mode, seed, phase: px.pack(img, 4, mode, seed, phase)),
               10: ((), np.uint32, lambda img, mode, seed, phase: ho.pack(img, "rgb10a2", mode, seed, phase)),
               16: ((3,), np.uint16, lambda img, mode, seed, phase: ho.pack(img, "rgb16", mode, seed, phase))}
    runs = {"pixels_pack_kernel": 0, "hdr_pack_kernel": 0}
    pixels = dict(runs)
    for W, H in t.SIZES:
        for img in t.images(W, H):
            for fmt, (tail, dtype, ref) in formats.items():
                kernel = "hdr_pack_kernel" if fmt >= 10 else "pixels_pack_kernel"
                for m, mode in enumerate(px.MODES):
                    for phase in t.PHASES:
                        seed = 0 if phase == 0 else 0xC0FFEE + phase
                        with open(os.path.join(work, "in.bin"), "wb") as f:
                            f.write(np.array([W, H, fmt, m], np.int32).tobytes())
                            f.write(np.array([seed, phase], np.uint32).tobytes())
                            f.write(np.ascontiguousarray(img, np.float32).tobytes())
                        subprocess.check_call([exe, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")])
                        got = np.fromfile(os.path.join(work, "out.bin"), dtype).reshape((H, W) + tail)
                        want = ref(img, mode, seed, phase)
                        if got.dtype != want.dtype or not (got == want).all():
                            raise SystemExit("differs from the restatement: %s" % ((W, H, fmt, mode, phase),))
                        runs[kernel] += 1
                        pixels[kernel] += W * H
    for kernel, ref in (("pixels_pack_kernel", "tests/pixels_ref.py"), ("hdr_pack_kernel", "tests/hdr_output_ref.py")):
        print("%s on the host under -fsanitize=address,undefined: %d runs, %d pixels, no report, every byte equal to %s" % (kernel, runs[kernel], pixels[kernel], ref))


if __name__ == "__main__":
    main()
