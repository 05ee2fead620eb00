"""Price and behaviour of the local exposure (include/digital_earth_local_exposure.h) -> profiles/local_exposure.md.

    for size in cfg2 cfg4; do for f in on off; do
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR/${size}_$f -o t -- python tools/local_exposure_price.py --trace $f --size $size
    done; done
    python tools/local_exposure_price.py --stats DIR        # per trace: the display-path kernels' durations, every kernel name with its calls
    python tools/local_exposure_price.py --views --scale 4  # the four preset views with the default settings: what the stage does to the displayed image

--trace: one frame of the view (cfg2: 1920x1080, cfg4: 3840x2160 sunset hurricane) at 4 spp, then --reps displays on the device (de_render_to_image:
no host copy).  "on": local exposure AND bloom on with their defaults, so that lx_*, bloom_* and display_kernel stand next to each other in one trace;
"off": neither ever turned on (no lx_ kernel may appear in that trace).  Run it under rocprofv3.
--views: per view at 1/scale of its BASELINE size and 64 spp, the luminance percentiles of the DISPLAYED image (Rec. 709 luminance of fetch_image(),
0 .. 1) with and without the stage, the gain's range in stops, and the share of pixels that are not light."""
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

PERCENTILES = (1, 5, 25, 50, 75, 95, 99)


def run_trace(args):
    r = make(args.size, 1)
    r.reset_framebuffer()
    accumulate(r, 4)
    if args.trace == "on":
        r.set_bloom(True)
        r.set_local_exposure(True, levels=args.levels)
    for _ in range(args.reps):
        r.render_to_image_device()
    r.synchronize()
    print(json.dumps(dict(view=args.size, size=list(r.image_res), feature=args.trace, displays=args.reps, settings=r.local_exposure)), flush=True)
    r.close()


def _short(kernel_name):
    return kernel_name.split("(")[0].replace("void ", "")


def run_stats(args):
    """Per *kernel_trace.csv under the directory: the durations of the display-path kernels (the first two displays are dropped as warm-up), the sum
    of the lx_ and of the bloom_ kernels per display, then every kernel of the trace with its number of calls."""
    for path in sorted(glob.glob(os.path.join(args.stats, "**", "*kernel_trace.csv"), recursive=True)):
        rows, calls = {}, {}
        for row in sorted(csv.DictReader(open(path)), key=lambda q: int(q["Start_Timestamp"])):
            k = _short(row["Kernel_Name"])
            calls[k] = calls.get(k, 0) + 1
            if any(s in k for s in ("lx_", "bloom_", "display_kernel")):
                rows.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
        print(os.path.relpath(path, args.stats))
        n_disp = sum(len(v) for k, v in rows.items() if "display_kernel" in k)
        skip = 2 if n_disp > 4 else 0
        sums = {"lx_": 0.0, "bloom_": 0.0}
        for k, us in sorted(rows.items()):
            per = len(us) // n_disp if n_disp and len(us) % n_disp == 0 else 0
            us = us[skip * max(per, 1):]
            print("  %-44s calls %4d  per display %2d  median %8.2f us  mean %8.2f us  min %8.2f us  max %8.2f us"
                  % (k, len(us), per, float(np.median(us)), float(np.mean(us)), float(np.min(us)), float(np.max(us))))
            for family in sums:
                if family in k:
                    sums[family] += float(np.median(np.array(us).reshape(-1, per).sum(axis=1))) if per else float(np.median(us))
        print("  per display, summed medians: lx_ %.2f us, bloom_ %.2f us" % (sums["lx_"], sums["bloom_"]))
        print("  kernels: " + ", ".join("%s x%d" % kv for kv in sorted(calls.items())))
        print("  lx_ kernels in this trace: %d" % sum(n for k, n in calls.items() if "lx_" in k))


def _luminance(a):
    return 0.2126 * a[..., 0] + 0.7152 * a[..., 1] + 0.0722 * a[..., 2]


def run_views(args):
    for name in args.configs:
        r = make(name, args.scale)
        r.reset_framebuffer()
        accumulate(r, 64)
        plain = _luminance(r.fetch_image().astype(np.float64))
        mean = r.fetch_hdr().astype(np.float64) / 64.0
        r.set_local_exposure(True)
        shown = _luminance(r.fetch_image().astype(np.float64))
        out = r.fetch_local_exposure_hdr().astype(np.float64)
        y0, y1 = _luminance(mean), _luminance(out)
        lit = (y0 >= 2.0 ** -24) & np.isfinite(y0)
        ev = np.log2(y1[lit] / y0[lit])
        print(json.dumps(dict(view=name, preset=VIEWS[name]["preset"] or "default", size=list(r.image_res), settings=r.local_exposure,
                              exposure=float(r.exposure[None]), not_light_share=float(1.0 - lit.mean()),
                              percentiles=list(PERCENTILES),
                              displayed_off=[float(v) for v in np.percentile(plain, PERCENTILES)],
                              displayed_on=[float(v) for v in np.percentile(shown, PERCENTILES)],
                              displayed_lit_off=[float(v) for v in np.percentile(plain[lit], PERCENTILES)],
                              displayed_lit_on=[float(v) for v in np.percentile(shown[lit], PERCENTILES)],
                              gain_ev_min=float(ev.min()), gain_ev_median=float(np.median(ev)), gain_ev_max=float(ev.max()),
                              burned_share=float((ev < -1e-3).mean()), dodged_share=float((ev > 1e-3).mean()))), flush=True)
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(VIEWS), choices=list(VIEWS))
    ap.add_argument("--trace", choices=["on", "off"])
    ap.add_argument("--size", choices=["cfg2", "cfg4"], default="cfg2")
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--stats", metavar="DIR")
    ap.add_argument("--views", action="store_true")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.trace:
        run_trace(args)
    if args.stats:
        run_stats(args)
    if args.views:
        run_views(args)


if __name__ == "__main__":
    main()
