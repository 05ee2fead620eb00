"""Price and behaviour of the history reprojection (include/digital_earth_history.h) -> profiles/history.md.

    for size in cfg2 cfg4; do for f in on off; do
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR/${size}_$f -o t -- python tools/history_price.py --trace $f --size $size
    done; done
    python tools/history_price.py --stats DIR          # per trace: history_blend_kernel next to display_kernel, every kernel name with its calls
    python tools/history_price.py --coverage --scale 4  # the four preset views: share of pixels with w > 0 after a one-pixel and a twenty-pixel yaw

--trace on | off --size cfg2 | cfg4: the workload of ONE kernel trace — a 4-spp frame of cfg2 (1920x1080) or cfg4 (3840x2160) and a display, a yaw of
1.5 pixels and a reset, a 1-spp frame, then --reps displays left on the device (de_render_to_image: no host copy), with the feature on (every one of
those displays reprojects the first frame's picture), or never turned on (no history_ kernel may appear in that trace).
--coverage: per view at 1/scale of its BASELINE size: 4 spp and a display, the yaw, a reset, 1 spp; the share of pixels whose blended weight exceeds
the frame's own sample count (w > 0).
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


def yaw(r, pixels):
    """Turn the look-at point about the up axis by `pixels` pixels of the image."""
    pos, look, up = (np.array(v[None], np.float64) for v in (r.camera_pos, r.look_at, r.up))
    a = pixels * 2.0 * float(r.fov[None]) / r.image_res[1]
    o = look - pos
    k = up / np.linalg.norm(up)
    o = o * np.cos(a) + np.cross(k, o) * np.sin(a) + k * np.dot(k, o) * (1.0 - np.cos(a))      # Rodrigues
    r.set_look_at(*(pos + o))


def run_trace(args):
    r = make(args.size, 1)
    if args.trace == "on":
        r.set_history(True)
    r.reset_framebuffer()
    accumulate(r, 4)
    r.render_to_image_device()
    yaw(r, 1.5)
    r.reset_framebuffer()
    accumulate(r, 1)
    for _ in range(args.reps):
        r.render_to_image_device()
    r.synchronize()
    W, H = r.image_res
    print(json.dumps(dict(view=args.size, size=[W, H], feature=args.trace, displays=args.reps + 1)), flush=True)
    r.close()


def _short(kernel_name):
    return kernel_name.split("(")[0].replace("void ", "")


def run_stats(args):
    """Per *kernel_trace.csv under the directory: the durations of history_blend_kernel, guide_kernel and display_kernel (the first two displays are
    dropped as warm-up), then every kernel of the trace with its number of calls — the feature-off traces must name no history_ kernel."""
    for path in sorted(glob.glob(os.path.join(args.stats, "**", "*kernel_trace.csv"), recursive=True)):
        rows, calls = {}, {}
        for row in sorted(csv.DictReader(open(path)), key=lambda q: int(q["Start_Timestamp"])):
            k = _short(row["Kernel_Name"])
            calls[k] = calls.get(k, 0) + 1
            if any(s in k for s in ("history_", "display_kernel", "guide_kernel")):
                rows.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
        print(os.path.relpath(path, args.stats))
        for k, us in sorted(rows.items()):
            us = us[2:] if len(us) > 4 else us
            print("  %-44s calls %4d  median %8.2f us  mean %8.2f us  min %8.2f us  max %8.2f us" % (k, len(us), float(np.median(us)), float(np.mean(us)), float(np.min(us)), float(np.max(us))))
        print("  kernels: " + ", ".join("%s x%d" % kv for kv in sorted(calls.items())))
        print("  history kernels in this trace: %d" % sum(n for k, n in calls.items() if "history_" in k))


def run_coverage(args):
    for name in args.configs:
        for pixels in (1.0, 20.0):
            r = make(name, args.scale)
            r.set_history(True)
            r.reset_framebuffer()
            accumulate(r, 4)
            r.fetch_image()
            yaw(r, pixels)
            r.reset_framebuffer()
            accumulate(r, 1)
            out = r.fetch_history_hdr()
            print(json.dumps(dict(view=name, preset=VIEWS[name]["preset"] or "default", size=list(r.image_res), yaw_pixels=pixels,
                                  share_with_history=float((out[..., 3] > 1.0).mean()), mean_weight=float(out[..., 3].mean()))), flush=True)
            r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(VIEWS), choices=list(VIEWS))
    ap.add_argument("--trace", choices=["on", "off"])
    ap.add_argument("--size", choices=["cfg2", "cfg4"], default="cfg2")
    ap.add_argument("--stats", metavar="DIR")
    ap.add_argument("--coverage", action="store_true")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.trace:
        run_trace(args)
    if args.stats:
        run_stats(args)
    if args.coverage:
        run_coverage(args)


if __name__ == "__main__":
    main()
