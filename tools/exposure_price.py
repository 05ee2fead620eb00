"""Price and behaviour of auto-exposure (include/digital_earth_exposure.h) -> profiles/auto_exposure.md.

    for size in cfg2 cfg4; do for f in on off; do
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR/${size}_$f -o t -- python tools/exposure_price.py --trace $f --size $size
    done; done
    python tools/exposure_price.py --stats DIR          # per trace: the display-path kernels' durations, and every kernel name with its calls
    python tools/exposure_price.py --ev --scale 4       # the metered EV of the four preset views

--trace on | off --size cfg2 | cfg4: the workload of ONE kernel trace — a 4-spp frame of cfg2 (1920x1080) or cfg4 (3840x2160), then --reps displays left
on the device (de_render_to_image: no host copy), with the feature on, or never turned on (no metering kernel may appear in that trace).  One size per
trace: the meter's grid is capped and the solve is one workgroup, so grids could not tell the sizes apart.  --stats names each trace by its directory.
--ev: per view at 1/scale of its BASELINE size, the metered EV (default settings) at 1 / 4 / 16 / 64 spp, raw and with the denoiser on, next to the
preset's hand-set exposure, with the share of pixels not metered (below 2^-24) and clipped.
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from adaptive_price import VIEWS, make  # noqa: E402
from denoise_price import accumulate  # noqa: E402


def run_trace(args):
    r = make(args.size, 1)
    r.reset_framebuffer()
    accumulate(r, 4)
    if args.trace == "on":
        r.set_auto_exposure(True)
    for _ in range(args.reps):
        r.render_to_image_device()
    r.synchronize()
    out = dict(view=args.size, size=list(r.image_res), feature=args.trace, displays=args.reps)
    if args.trace == "on":
        m = r.metering()
        out.update(ev=m["ev"], metered=m["metered"], below=m["below"], clipped=m["clipped"])
    print(json.dumps(out), flush=True)
    r.close()


def _short(kernel_name):
    return kernel_name.split("(")[0].replace("void ", "")


def run_stats(args):
    """Per *kernel_trace.csv under the directory: the durations of the display-path kernels (the first two calls of each are dropped as warm-up), then
    every kernel of the trace with its number of calls — the feature-off traces must name no meter_ kernel."""
    for path in sorted(glob.glob(os.path.join(args.stats, "**", "*kernel_trace.csv"), recursive=True)):
        rows, calls = {}, {}
        for row in csv.DictReader(open(path)):
            k = _short(row["Kernel_Name"])
            calls[k] = calls.get(k, 0) + 1
            if any(s in k for s in ("meter_", "display_kernel")):
                rows.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
        print(os.path.relpath(path, args.stats))
        for k, us in sorted(rows.items()):
            us = us[2:] if len(us) > 4 else us
            print("  %-40s calls %3d  median %8.2f us  mean %8.2f us  min %8.2f us  max %8.2f us" % (k, len(us), float(np.median(us)), float(np.mean(us)), float(np.min(us)), float(np.max(us))))
        print("  kernels: " + ", ".join("%s x%d" % kv for kv in sorted(calls.items())))
        print("  meter kernels in this trace: %d" % sum(n for k, n in calls.items() if "meter_" in k))


def run_ev(args):
    steps = (1, 4, 16, 64)
    for name in args.configs:
        r = make(name, args.scale)
        manual = float(r.exposure[None])
        r.set_auto_exposure(True)
        rows = []
        for spp in steps:
            row = dict(spp=spp)
            for tag, dn in (("raw", False), ("denoised", True)):
                r.set_denoise(dn)
                r.set_auto_exposure(True)
                r.reset_framebuffer()
                accumulate(r, spp)
                r.fetch_image()
                m = r.metering()
                n = float(m["metered"] + m["below"])
                row[tag] = dict(ev=m["ev"], mean_log2=m["mean_log2"], below=m["below"] / n, clipped=m["clipped"] / n)
            rows.append(row)
        print(json.dumps(dict(view=name, preset=VIEWS[name]["preset"] or "default", size=list(r.image_res), manual_exposure=manual, rows=rows)), flush=True)
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(VIEWS), choices=list(VIEWS))
    ap.add_argument("--trace", choices=["on", "off"])
    ap.add_argument("--size", choices=["cfg2", "cfg4"], default="cfg2")
    ap.add_argument("--stats", metavar="DIR")
    ap.add_argument("--ev", action="store_true")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.trace:
        run_trace(args)
    if args.stats:
        run_stats(args)
    if args.ev:
        run_ev(args)


if __name__ == "__main__":
    main()
