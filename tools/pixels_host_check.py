"""pixels_pack_kernel's source on the HOST under the address and undefined-behaviour sanitizers: builds tools/pixels_host_check.cpp
(a stand-alone program that includes csrc/pixels_kernels.hip and runs its two halves one workgroup at a time), feeds it the inputs of
tests/test_gpu_pixels.py::test_kernel_equals_the_restatement_byte_for_byte at the three sizes — both channel counts, the three modes, the three
phases — and compares what it writes with the numpy restatement (tests/pixels_ref.py) byte for byte.  Needs a C++ compiler and no GPU.

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
    import pixels_ref as px
    import test_gpu_pixels as t
    work = args.keep or tempfile.mkdtemp(prefix="pixels_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "pixels_host_check")
    subprocess.check_call([args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-x", "c++", os.path.join(ROOT, "tools", "pixels_host_check.cpp"), "-o", exe])
    runs = pixels = 0
    for W, H in t.SIZES:
        for img in t.images(W, H):
            for channels in (3, 4):
                for m, mode in enumerate(px.MODES):
                    for phase in t.PHASES:
                        seed = 0 if phase == 0 else 0xC0FFEE + phase
                        with open(os.path.join(work, "in.bin"), "wb") as f:
                            f.write(np.array([W, H, channels, m], np.int32).tobytes())
                            f.write(np.array([seed, phase], np.uint32).tobytes())
                            f.write(np.ascontiguousarray(img, np.float32).tobytes())
                        subprocess.check_call([exe, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")])
                        got = np.fromfile(os.path.join(work, "out.bin"), np.uint8).reshape(H, W, channels)
                        want = px.pack(img, channels, mode, seed, phase)
                        if not (got == want).all():
                            raise SystemExit("differs from tests/pixels_ref.py: %s" % ((W, H, channels, mode, phase),))
                        runs += 1
                        pixels += W * H
    print("pixels_pack_kernel on the host under -fsanitize=address,undefined: %d runs, %d pixels, no report, every byte equal to tests/pixels_ref.py" % (runs, pixels))


if __name__ == "__main__":
    main()
