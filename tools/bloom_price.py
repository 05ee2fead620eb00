"""Price and behaviour of the bloom (include/digital_earth_bloom.h) -> profiles/bloom.md.

    for size in cfg2 cfg4; do for f in on off; do
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR/${size}_$f -o t -- python tools/bloom_price.py --trace $f --size $size
    done; done
    python tools/bloom_price.py --stats DIR          # per trace: the display-path kernels' durations, the pyramid's tail, every kernel name with its calls
    python tools/bloom_price.py --pipelined          # the window loop at fetch_image(lag=1), bloom on against off, alternating
    python tools/bloom_price.py --views --scale 4    # the four preset views with the default settings: what the bloom moves

--trace on | off --size cfg2 | cfg4: the workload of ONE kernel trace — a 4-spp frame of cfg2 (1920x1080) or cfg4 (3840x2160), then --reps displays left
on the device (de_render_to_image: no host copy), with the feature on (--levels, default 6), or never turned on (no bloom kernel may appear in that
trace).  --stats names each trace by its directory; the launches of one display come in a fixed order (down0, the levels down, the levels up, the
composite), so a call's level is its position: the tail is every launch whose output is level 3 or coarser.
--pipelined: per-frame host time of accumulate(1) + fetch_image(lag=1) over --frames frames, bloom off / on alternating --rounds times in one process.
--views: per view at 1/scale of its BASELINE size and 64 spp, the share of the image's light that the default bloom moves, the relative glow
well away from the bright regions, and how much of the displayed image changes by more than one 8-bit step.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from adaptive_price import VIEWS, make  # noqa: E402
from denoise_price import accumulate  # noqa: E402


def levels_used(W, H, levels):
    L, w, h = 0, W, H
    while L < levels:
        w, h = (w + 1) >> 1, (h + 1) >> 1
        if min(w, h) < 2 and L >= 1:
            break
        L += 1
    return L


def run_trace(args):
    r = make(args.size, 1)
    r.reset_framebuffer()
    accumulate(r, 4)
    if args.trace == "on":
        r.set_bloom(True, levels=args.levels)
    for _ in range(args.reps):
        r.render_to_image_device()
    r.synchronize()
    W, H = r.image_res
    print(json.dumps(dict(view=args.size, size=[W, H], feature=args.trace, displays=args.reps,
                          levels=levels_used(W, H, args.levels) if args.trace == "on" else 0)), flush=True)
    r.close()


def _short(kernel_name):
    return kernel_name.split("(")[0].replace("void ", "")


def _line(k, us):
    return "  %-44s calls %4d  median %8.2f us  mean %8.2f us  min %8.2f us  max %8.2f us" % (k, len(us), float(np.median(us)), float(np.mean(us)), float(np.min(us)), float(np.max(us)))


def run_stats(args):
    """Per *kernel_trace.csv under the directory: the durations of the display-path kernels (the first two displays are dropped as warm-up), the
    levels of the pyramid one by one and the tail's sum next to the composite, then every kernel of the trace with its number of calls — the
    feature-off traces must name no bloom_ kernel."""
    for path in sorted(glob.glob(os.path.join(args.stats, "**", "*kernel_trace.csv"), recursive=True)):
        rows, calls = {}, {}
        for row in sorted(csv.DictReader(open(path)), key=lambda q: int(q["Start_Timestamp"])):
            k = _short(row["Kernel_Name"])
            calls[k] = calls.get(k, 0) + 1
            if any(s in k for s in ("bloom_", "display_kernel")):
                rows.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
        print(os.path.relpath(path, args.stats))
        n_disp = sum(len(v) for k, v in rows.items() if "display_kernel" in k)
        skip = 2 if n_disp > 4 else 0
        med = {}
        for k, us in sorted(rows.items()):
            per = len(us) // n_disp if n_disp and len(us) % n_disp == 0 else 0
            us = us[skip * max(per, 1):]
            print(_line(k, us))
            med[k] = (us, per)
        down = next((v for k, v in med.items() if k.startswith("bloom_down_kernel")), None)
        up = next((v for k, v in med.items() if k.startswith("bloom_up_kernel")), None)
        comp = next((v for k, v in med.items() if k.startswith("bloom_composite_kernel")), None)
        if down and up and comp and down[1] and up[1] == down[1]:
            per = down[1]                      # L - 1 launches of each per display
            L = per + 1
            d = np.array(down[0]).reshape(-1, per)      # column k makes D_{k+2}
            u = np.array(up[0]).reshape(-1, per)        # column k makes U_{L-1-k}
            for k in range(per):
                print("    down to D_%-2d median %7.2f us      up to U_%-2d median %7.2f us" % (k + 2, float(np.median(d[:, k])), L - 1 - k, float(np.median(u[:, k]))))
            tail = d[:, 1:].sum(axis=1) + u[:, :max(L - 3, 0)].sum(axis=1)      # outputs D_3 .. D_L and U_{L-1} .. U_3
            print("  tail (every launch whose output is level 3 or coarser: %d launches): median %.2f us; composite: median %.2f us"
                  % ((per - 1) + max(L - 3, 0), float(np.median(tail)), float(np.median(comp[0]))))
        total = sum(float(np.median(np.array(us).reshape(-1, per).sum(axis=1))) if per else float(np.median(us)) for k, (us, per) in med.items() if "bloom_" in k)
        print("  bloom kernels per display, summed medians: %.2f us" % total)
        print("  kernels: " + ", ".join("%s x%d" % kv for kv in sorted(calls.items())))
        print("  bloom kernels in this trace: %d" % sum(n for k, n in calls.items() if "bloom_" in k))


def run_pipelined(args):
    r = make(args.size, 1)

    def loop(on):
        r.set_bloom(on)
        r.reset_framebuffer()
        for _ in range(8):                     # warm-up: the ring buffers, the code objects
            r.accumulate(1)
            r.fetch_image(copy=False, lag=1)
        r.fetch_pending()
        r.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.frames):
            r.accumulate(1)
            r.fetch_image(copy=False, lag=1)
        r.fetch_pending()
        r.synchronize()
        return (time.perf_counter() - t0) / args.frames * 1e3
    ms = {False: [], True: []}
    for _ in range(args.rounds):
        for on in (False, True):
            ms[on].append(loop(on))
    print(json.dumps(dict(view=args.size, size=list(r.image_res), frames=args.frames, lag=1, off_ms=ms[False], on_ms=ms[True],
                          off_median=float(np.median(ms[False])), on_median=float(np.median(ms[True])),
                          difference_us=1e3 * float(np.median(ms[True]) - np.median(ms[False])))), flush=True)
    r.close()


def run_views(args):
    for name in args.configs:
        r = make(name, args.scale)
        r.reset_framebuffer()
        accumulate(r, 64)
        plain = r.fetch_image().astype(np.float64)
        mean = r.fetch_hdr().astype(np.float64) / 64.0
        r.set_bloom(True)
        s = r.bloom()
        shown = r.fetch_image().astype(np.float64)
        out = r.fetch_bloom_hdr().astype(np.float64)
        Y = lambda a: 0.2126 * a[..., 0] + 0.7152 * a[..., 1] + 0.0722 * a[..., 2]
        y0, y1 = Y(mean), Y(out)
        dark = y0 < 1e-3 * y0.max()            # well away from the light: what the glow lifts there, against the frame's peak and its mean
        step = np.abs(shown - plain).max(axis=-1)
        print(json.dumps(dict(view=name, preset=VIEWS[name]["preset"] or "default", size=list(r.image_res), settings=s,
                              energy_ratio=float(y1.sum() / y0.sum()), peak=float(y0.max()), mean=float(y0.mean()),
                              dark_share=float(dark.mean()), glow_in_dark_over_mean=float(y1[dark].mean() / y0.mean()) if dark.any() else None,
                              peak_kept=float(y1.max() / y0.max()),
                              display_changed_over_1_255=float((step > 1.0 / 255.0).mean()), display_changed_over_4_255=float((step > 4.0 / 255.0).mean()),
                              display_max_change=float(step.max()), display_mean_change=float(step.mean()))), flush=True)
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(VIEWS), choices=list(VIEWS))
    ap.add_argument("--trace", choices=["on", "off"])
    ap.add_argument("--size", choices=["cfg2", "cfg4"], default="cfg2")
    ap.add_argument("--levels", type=int, default=6)
    ap.add_argument("--stats", metavar="DIR")
    ap.add_argument("--pipelined", action="store_true")
    ap.add_argument("--views", action="store_true")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.trace:
        run_trace(args)
    if args.stats:
        run_stats(args)
    if args.pipelined:
        run_pipelined(args)
    if args.views:
        run_views(args)


if __name__ == "__main__":
    main()
