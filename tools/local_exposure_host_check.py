"""The four local exposure kernels' source on the HOST under the address and undefined-behaviour sanitizers: builds
tools/local_exposure_host_check.cpp (a stand-alone program that includes csrc/local_exposure_kernels.hip and csrc/de_math.h and runs the kernels'
phases one workgroup at a time), feeds it the inputs and settings of tests/test_gpu_local_exposure.py::test_hook_equals_the_restatement_bit_for_bit at
the four sizes, through the float4 and the scalar loads, and compares what it writes with the numpy restatement (tests/local_exposure_ref.py) bit for
bit — the restatement's logarithm and power of two are the same program's de_log and de_pow.  Needs a C++ compiler and no GPU; it is never run on one.

    python tools/local_exposure_host_check.py [--cxx g++] [--keep DIR]
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
    import local_exposure_ref as lx
    import test_gpu_local_exposure as t
    work = args.keep or tempfile.mkdtemp(prefix="local_exposure_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "local_exposure_host_check")
    subprocess.check_call([args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tools", "host_shim"), "-x", "c++", os.path.join(ROOT, "tools", "local_exposure_host_check.cpp"), "-o", exe])
    fin, fout = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")

    def math(which):
        def fn(x):
            x = np.ascontiguousarray(x, np.float32)
            x.tofile(fin)
            subprocess.check_call([exe, which, fin, fout])
            return np.fromfile(fout, np.float32).reshape(x.shape)
        return fn
    dm = dict(log=math("log"), pow2=math("pow2"))
    runs = pixels = 0
    for W, H in t.SIZES:
        for name, mean in t.inputs(W, H).items():
            for setting, kw in t.SETTINGS.items():
                s = dict(lx.DEFAULTS, **kw)
                want = lx.local_exposure(mean, 1, t.EXPOSURE_SCALE, **kw, **dm)[0]
                for vec in (1, 0):
                    with open(fin, "wb") as f:
                        f.write(np.array([W, H, s["levels"], vec], np.int32).tobytes())
                        f.write(np.array([t.EXPOSURE_SCALE, s["highlights"], s["shadows"], s["sigma"], s["max_ev"], s["key"]], np.float32).tobytes())
                        f.write(np.ascontiguousarray(mean.transpose(1, 0, 2), np.float32).tobytes())
                    subprocess.check_call([exe, "run", fin, fout])
                    got = np.fromfile(fout, np.float32).reshape(H, W, 3).transpose(1, 0, 2)
                    nan = np.isnan(want)
                    if not ((np.isnan(got) == nan).all() and (got.view(np.uint32) == want.view(np.uint32))[~nan].all()):
                        raise SystemExit("differs from tests/local_exposure_ref.py: %s" % ((W, H, name, setting, vec),))
                    runs += 1
                    pixels += W * H
    print("lx_down0 / lx_down / lx_up / lx_apply on the host under -fsanitize=address,undefined: %d runs, %d pixels, no report, every bit equal to "
          "tests/local_exposure_ref.py" % (runs, pixels))


if __name__ == "__main__":
    main()
