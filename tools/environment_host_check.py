"""The capture kernel of the scene-linear panorama on the HOST under the address and undefined-behaviour sanitizers: builds
tools/environment_host_check.cpp (a stand-alone program that includes csrc/environment_body.h and replays the launch workgroup by workgroup, thread
by thread, on heap blocks of exactly their sizes) and compares the slot it writes with numpy: sums / count, transposed — N = 16 (one partial tile),
48 (2 x 2 tiles, the last partial), 64 (whole tiles) and 40 (no multiple of 16), with the frame's count and with a count per 8 x 8 tile.  Needs a C++
compiler and no GPU; nothing sanitized is loaded into Python.

    python tools/environment_host_check.py [--cxx g++] [--keep DIR]
"""
import argparse
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX", "g++"))
    ap.add_argument("--keep", metavar="DIR")
    args = ap.parse_args()
    work = args.keep or tempfile.mkdtemp(prefix="environment_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "environment_host_check")
    subprocess.check_call([args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "environment_host_check.cpp"), "-o", exe])
    F = np.float32
    rng = np.random.default_rng(26)
    runs = values = 0
    for N in (16, 48, 64, 40):
        for per_tile in (False, True):
            sums = (rng.random((N, N, 3), dtype=F) * F(1e4) - F(100.0)).astype(F)      # [j][i][c]
            counts = rng.integers(1, 40, (N // 8, N // 8)).astype(np.int32)            # [j / 8][i / 8]
            samples = 7
            with open(os.path.join(work, "in.bin"), "wb") as fh:
                fh.write(np.array([N, samples, int(per_tile)], np.int32).tobytes() + sums.tobytes())
                if per_tile:
                    fh.write(counts.tobytes())
            subprocess.check_call([exe, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")])
            got = np.fromfile(os.path.join(work, "out.bin"), F).reshape(N, N, 3)      # [i][j][c]
            div = np.repeat(np.repeat(counts, 8, axis=0), 8, axis=1).astype(F)[..., None] if per_tile else F(samples)
            want = np.ascontiguousarray((sums / div).astype(F).transpose(1, 0, 2))
            if not (got.view(np.uint32) == want.view(np.uint32)).all():
                raise SystemExit("differs from sums / count transposed: N %d, per tile %s" % (N, per_tile))
            runs += 1
            values += got.size
    print("the capture's two phases on the host under -fsanitize=address,undefined: %d runs, %d slot values, no report, every value equal to sums / count transposed bit for bit"
          % (runs, values))


if __name__ == "__main__":
    main()
