"""What the look LUTs cost (include/digital_earth_look.h; the tables of profiles/look.md).

    python tools/look_price.py --calls [--repeats 5] [--n 300]       de_render_to_image on one 1920x1080 context: the stage off (two arms: their
                                                                     difference is the spread), then on for 17^3 / 33^3 / 65^3 x trilinear / tetrahedral,
                                                                     a 1024-entry shaper alone and ahead of a 33^3 cube
    python tools/look_price.py --off [--root DIR]                    the stage-off arm alone, with the package of another source tree (DIR: a checkout
                                                                     of the parent commit, built): one JSON line
    python tools/look_price.py --ab PARENT_DIR [--rounds 3]          --off in fresh processes, this tree and PARENT_DIR in turn
    python tools/look_price.py --trace                               launches left on the device, for `rocprofv3 --kernel-trace --stats -- python ...`

Host clock around work that ends in a device synchronise; the arms alternate inside every repeat; every arm is warmed up first (the first pass over
the arms is dropped).  Prints one JSON line per mode."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080
ARMS = [("cube %d %s" % (n, i), n, i) for n in (17, 33, 65) for i in ("trilinear", "tetrahedral")]


def _summary(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def _renderer(root):
    sys.path.insert(0, root)
    from digital_earth_amd.renderer import Renderer
    r = Renderer((W, H), (0, 1, 0), texture_source="constant")      # the display path reads the sums and the LUTs only
    r.copy_textures()
    rng = np.random.default_rng(0)
    r.upload_hdr((np.exp2(rng.uniform(-9.0, 3.0, (W, H, 1))) * rng.uniform(0.3, 1.6, (W, H, 3))).astype(np.float32), 4)
    return r


def _time(r, n):
    r.render_to_image_device()
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        r.render_to_image_device()
    r.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def _noise(kind, n):
    from digital_earth_amd import cube
    return cube.Cube(kind, n, np.random.default_rng(n).uniform(0.0, 1.0, cube.rows(kind, n) * 3).astype(np.float32))


def calls(args):
    r = _renderer(HERE)
    arms = [("off a", None), ("off b", None)] + [(name, dict(cube=_noise("3d", n), interpolation=i)) for name, n, i in ARMS]
    arms += [("shaper 1024", dict(shaper=_noise("1d", 1024))), ("shaper 1024 + cube 33 tetrahedral", dict(shaper=_noise("1d", 1024), cube=_noise("3d", 33)))]
    times = {name: [] for name, _ in arms}
    for rep in range(args.repeats + 1):
        for name, kw in arms:
            if kw is None:
                r.set_look(enabled=False)
            else:
                r.set_look(**kw)
            t = _time(r, args.n)
            if rep:
                times[name].append(t)
    print(json.dumps(dict(what="microseconds per de_render_to_image back to back, 1920x1080; the image is noise: the gathers are spread over the whole table",
                          n=args.n, repeats=args.repeats, arms={k: _summary(x) for k, x in times.items()})), flush=True)
    r.close()


def off(args):
    r = _renderer(os.path.abspath(args.root))
    xs = [_time(r, args.n) for _ in range(args.repeats + 1)][1:]
    print(json.dumps(dict(what="microseconds per de_render_to_image, stage off", root=os.path.abspath(args.root), n=args.n, **_summary(xs))), flush=True)
    r.close()


def ab(args):
    trees = [("this tree", HERE), ("parent", os.path.abspath(args.ab))]
    got = {name: [] for name, _ in trees}
    for _ in range(args.rounds):
        for name, root in trees:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--off", "--root", root, "--n", str(args.n), "--repeats", str(args.repeats)],
                                 check=True, capture_output=True, text=True, timeout=300).stdout
            got[name].append(json.loads(out.strip().splitlines()[-1])["median"])
    print(json.dumps(dict(what="microseconds per de_render_to_image with the stage off: median of each fresh process, the two trees in turn", rounds=args.rounds,
                          arms=got)), flush=True)


def trace(args):
    r = _renderer(HERE)
    for _ in range(40):
        r.render_to_image_device()
    for name, n, i in ARMS:
        r.set_look(cube=_noise("3d", n), interpolation=i)
        for _ in range(40):
            r.render_to_image_device()
    r.synchronize()
    print(json.dumps(dict(what="40 launches of display_kernel alone, then 40 of display_kernel + look_apply_kernel per arm, in this order", arms=[a[0] for a in ARMS])), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--off", action="store_true")
    ap.add_argument("--ab", metavar="PARENT_DIR")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n", type=int, default=300)
    a = ap.parse_args()
    if a.calls:
        calls(a)
    if a.off:
        off(a)
    if a.ab:
        ab(a)
    if a.trace:
        trace(a)
