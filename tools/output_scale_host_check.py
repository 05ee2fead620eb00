"""The output scaling's source on the HOST under the address and undefined-behaviour sanitizers: builds
tools/output_scale_host_check.cpp (a stand-alone program that includes csrc/output_scale_kernels.hip and runs the table builder and the two passes one
workgroup at a time), feeds it the inputs of tests/test_gpu_output_scale.py::test_kernel_equals_the_restatement_bit_for_bit at its six size pairs plus
the extreme ratios (1/8 and 8 on both axes, and one against the other), all four filters, and compares what it writes with the numpy restatement
(tests/output_scale_ref.py) bit for bit.  Needs a C++ compiler and no GPU.

    python tools/output_scale_host_check.py [--cxx g++] [--keep DIR]
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

EXTREME = [((128, 64), (16, 8)), ((16, 8), (128, 64)), ((128, 8), (16, 64)), ((16, 64), (128, 8)), ((16, 1024), (16, 128)), ((16, 8), (16, 8))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "g++"))
    ap.add_argument("--keep", metavar="DIR")
    args = ap.parse_args()
    import output_scale_ref as ref
    import test_gpu_output_scale as t
    work = args.keep or tempfile.mkdtemp(prefix="output_scale_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "output_scale_host_check")
    subprocess.check_call([args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-x", "c++", os.path.join(ROOT, "tools", "output_scale_host_check.cpp"), "-o", exe])
    runs = values = 0
    for (W, H), (ow, oh) in list(t.PAIRS) + EXTREME:
        for img in t.images(W, H):
            for f, name in enumerate(ref.FILTERS):
                with open(os.path.join(work, "in.bin"), "wb") as fh:
                    fh.write(np.array([W, H, ow, oh, f], np.int32).tobytes())
                    fh.write(np.ascontiguousarray(img, np.float32).tobytes())
                subprocess.check_call([exe, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")])
                got = np.fromfile(os.path.join(work, "out.bin"), np.float32).reshape(ow, oh, 3)
                want = ref.resample(img, (ow, oh), name)
                same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
                if not same.all():
                    raise SystemExit("differs from tests/output_scale_ref.py: %s" % (((W, H), (ow, oh), name),))
                runs += 1
                values += got.size
    print("output scaling on the host under -fsanitize=address,undefined: %d runs, %d output values, no report, every value equal to tests/output_scale_ref.py bit for bit"
          % (runs, values))


if __name__ == "__main__":
    main()
