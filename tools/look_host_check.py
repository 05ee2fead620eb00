"""look_apply_kernel's source on the HOST under the address and undefined-behaviour sanitizers: builds tools/look_host_check.cpp (a
stand-alone program that includes csrc/look_kernels.hip and runs every thread of every workgroup), runs its own sweep, then feeds it the chains and
pixels of tests/test_gpu_look.py::test_kernel_equals_the_restatement — both interpolations, the three strengths — and compares what it writes with
the numpy restatement (tests/look_ref.py) byte for byte.  Needs a C++ compiler and no GPU.

    python tools/look_host_check.py [--cxx g++] [--keep DIR] [--counts 5 257 4100]
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


def write_case(path, x, cube, shaper, strength, interpolation):
    f32 = np.float32
    zeros, ones = (0.0,) * 3, (1.0,) * 3
    with open(path, "wb") as f:
        f.write(np.array([x.shape[0]], np.uint64).tobytes())
        f.write(np.array([shaper.size if shaper else 0, cube.size if cube else 0, 1 if interpolation == "tetrahedral" else 0], np.int32).tobytes())
        f.write(np.array((strength,) + (shaper.domain_min + shaper.domain_max if shaper else zeros + ones)
                         + (cube.domain_min + cube.domain_max if cube else zeros + ones), f32).tobytes())
        if shaper:
            f.write(np.frombuffer(shaper.table, dtype=f32).tobytes())
        if cube:
            f.write(np.frombuffer(cube.table, dtype=f32).tobytes())
        f.write(np.ascontiguousarray(x, f32).tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "g++"))
    ap.add_argument("--keep", metavar="DIR")
    ap.add_argument("--counts", type=int, nargs="*", default=[5, 257, 4100])
    args = ap.parse_args()
    import look_ref as lr
    import test_gpu_look as t
    work = args.keep or tempfile.mkdtemp(prefix="look_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "look_host_check")
    subprocess.check_call([args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-x", "c++", os.path.join(ROOT, "tools", "look_host_check.cpp"), "-o", exe])
    subprocess.check_call([exe])
    runs = pixels = 0
    src, dst = os.path.join(work, "in.bin"), os.path.join(work, "out.bin")
    for n in args.counts:
        x = t.pixels(n)
        for spec in t.CHAINS:
            chain = t._chain(spec)
            for interpolation in (lr.INTERPOLATIONS if "cube" in chain else ("tetrahedral",)):
                for s in t.STRENGTHS:
                    write_case(src, x, chain.get("cube"), chain.get("shaper"), s, interpolation)
                    subprocess.check_call([exe, src, dst])
                    got = np.fromfile(dst, np.float32).reshape(n, 3)
                    want = lr.apply(x, strength=s, interpolation=interpolation, **chain)
                    if not (got.view(np.uint32) == want.view(np.uint32)).all():
                        raise SystemExit("differs from tests/look_ref.py: %s" % ((n, spec, interpolation, s),))
                    runs += 1
                    pixels += n
    print("look_apply_kernel on the host under -fsanitize=address,undefined: %d runs, %d pixels, no report, every byte equal to tests/look_ref.py" % (runs, pixels))


if __name__ == "__main__":
    main()
