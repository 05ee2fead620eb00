"""The panorama stage's per-pixel body on the HOST under the address and undefined-behaviour sanitizers: builds
tools/panorama_host_check.cpp (a stand-alone program that includes csrc/panorama_body.h and runs it over every output pixel on heap blocks of exactly
their sizes), feeds it the cases of tests/test_gpu_panorama.py::test_kernel_equals_the_restatement_bit_for_bit — random faces of N = 16, both
projections, partial tiles, S = 1 ... 3, aprons 1 and 4, an oblique basis — and compares what it writes with the numpy restatement
(tests/panorama_ref.py) bit for bit.  Every case runs a second time through the row-major store of the scene-linear panorama (DESIGN.md §26:
pano_pixel_rows, with the tables staged tile by tile as environment_kernel stages them) and must give the same image transposed; the shapes of
tests/panorama_ref.py's MULTI_TILE at S = 4 run that side alone.  Needs a C++ compiler and no GPU; nothing sanitized is loaded into Python.

    python tools/panorama_host_check.py [--cxx g++] [--keep DIR]
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
    import panorama_ref as ref
    import test_gpu_panorama as t
    work = args.keep or tempfile.mkdtemp(prefix="panorama_host_")
    os.makedirs(work, exist_ok=True)
    exe = os.path.join(work, "panorama_host_check")
    subprocess.check_call([args.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "panorama_host_check.cpp"), "-o", exe])
    F = np.float32
    runs = values = 0
    for size, projection, aperture in t.OUTPUTS + ref.MULTI_TILE:
        multi = (size, projection, aperture) in ref.MULTI_TILE
        for apron in t.APRONS:
            for S in ((4,) if multi else t.SUPERSAMPLES):
                for basis in (None, t.OBLIQUE):
                    faces = t.random_faces(t.N, seed=S + 10 * apron)
                    fov, scale, half, m = ref.consts(t.N, apron, aperture, basis)
                    (sl, cl), (st, ct) = ref.tables(size[0], S, 2.0 * np.pi), ref.tables(size[1], S, np.pi)
                    with open(os.path.join(work, "in.bin"), "wb") as fh:
                        fh.write(np.array([t.N, size[0], size[1], S, int(projection == "fisheye")], np.int32).tobytes())
                        fh.write(np.array([fov, scale, half], F).tobytes() + np.ascontiguousarray(m, F).tobytes())
                        for tab in (sl, cl, st, ct):
                            fh.write(np.ascontiguousarray(tab, F).tobytes())
                        fh.write(np.ascontiguousarray(faces, F).tobytes())
                    want = ref.panorama(faces, size, projection, aperture, apron, S, basis)
                    for rows in ((True,) if multi else (False, True)):
                        subprocess.check_call([exe, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")] + (["rows"] if rows else []))
                        got = np.fromfile(os.path.join(work, "out.bin"), F)
                        got = np.ascontiguousarray(got.reshape(size[1], size[0], 3).transpose(1, 0, 2)) if rows else got.reshape(size[0], size[1], 3)
                        if not (got.view(np.uint32) == want.view(np.uint32)).all():
                            raise SystemExit("differs from tests/panorama_ref.py: %s" % ((size, projection, aperture, apron, S, basis is not None, rows),))
                        runs += 1
                        values += got.size
    print("the panorama body on the host under -fsanitize=address,undefined: %d runs, %d output values, no report, every value equal to tests/panorama_ref.py bit for bit"
          % (runs, values))


if __name__ == "__main__":
    main()
