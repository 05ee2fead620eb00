"""Price of the 8-bit pixel output (include/digital_earth_pixels.h) -> profiles/pixels.md.

    python tools/pixels_price.py --loop [--float-only]      # ms per frame of the window loop, lag 0 ... 3 (defaults: --frames 100 --warmup 20 --repeats 5)
    python tools/pixels_price.py --save                     # host time of save()'s conversion, old against new (--repeats 5)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/pixels_price.py --trace
    python tools/pixels_price.py --stats DIR                                            # pixels_pack_kernel next to display_kernel

--loop: BASELINE cfg2's view at 1920x1080, accumulate(1) per frame and a fetch of what is displayed as a zero-copy view: the float image
(fetch_image), RGBA8 and RGB8 (fetch_pixels), each truncated and dithered, at lag 0, 1, 2 and 3.  One run = a reset, --warmup frames, then --frames
timed frames by the host clock, ended by draining the ring and a device synchronise.  The runs of all arms alternate inside every repeat, so that a
drift of the machine lands on every arm; each arm reports the median, the minimum and the maximum of its repeats.  --float-only uses nothing this
feature added, so a copy of this file in the tools/ of a checkout of the parent commit gives the comparison on the same machine.
--save: a screenshot's conversion at 1920x1080 — the previous expression (clip * 255, cast, transpose, flip, made contiguous for the writer) on a
fetched float image against the writer's unpack of RGBA8 bytes, and against save()'s whole new path (the held float image through the pack kernel,
then that unpack); the synchronous fetches themselves are timed too.
--trace: the workload of one kernel trace: 40 conversions of each of RGBA8 and RGB8, truncated and dithered, left on the device.
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

from adaptive_price import make  # noqa: E402

ARMS = [("float32 (W, H, 3)", None), ("RGBA8 truncate", (4, "truncate")), ("RGBA8 dither", (4, "dither")), ("RGB8 truncate", (3, "truncate")), ("RGB8 dither", (3, "dither"))]


def one_run(r, arm, lag, warmup, frames):
    fetch = (lambda: r.fetch_image(copy=False, lag=lag)) if arm is None else (lambda: r.fetch_pixels(copy=False, lag=lag))
    drain = (lambda: r.fetch_pending(copy=False)) if arm is None else (lambda: r.fetch_pending(copy=False, pixels=True))
    if arm is not None:
        r.set_pixels(arm[0], arm[1], seed=1, animate=True)
    r.reset_framebuffer()
    for _ in range(warmup):
        r.accumulate(1)
        fetch()
    drain()
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        r.accumulate(1)
        fetch()
    drain()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e3 / frames


def run_loop(args):
    r = make("cfg2", 1)
    arms = ARMS[:1] if args.float_only else ARMS
    ms = {(name, lag): [] for name, _ in arms for lag in range(4)}
    for _ in range(args.repeats):
        for lag in range(4):
            for name, arm in arms:
                ms[(name, lag)].append(one_run(r, arm, lag, args.warmup, args.frames))
    for (name, lag), v in ms.items():
        print(json.dumps(dict(arm=name, lag=lag, size=list(r.image_res), frames=args.frames, repeats=args.repeats, ms_per_frame_median=round(float(np.median(v)), 3),
                              ms_min=round(float(np.min(v)), 3), ms_max=round(float(np.max(v)), 3))), flush=True)
    r.close()


def _median_ms(fn, repeats):
    fn()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median=round(float(np.median(t)), 3), min=round(float(np.min(t)), 3), max=round(float(np.max(t)), 3))


def run_save(args):
    """What EarthViewer.save does between the picture it holds and the image writer: before, the host expression on the float image; now, the pack
    kernel on the held image (Renderer.debug_pixels: upload, kernel, download) and the writer's unpack of its bytes (earth_viewer._rgb_picture)."""
    from PIL import Image
    from digital_earth_amd.earth_viewer import _rgb_picture
    r = make("cfg2", 1)
    r.accumulate(4)
    image, px = r.fetch_image(), r.fetch_pixels()
    old = lambda: Image.fromarray((np.clip(image, 0.0, 1.0) * 255).astype(np.uint8).transpose(1, 0, 2)[::-1])      # noqa: E731
    new = lambda: _rgb_picture(px)      # noqa: E731
    both = lambda: _rgb_picture(r.debug_pixels(image))      # noqa: E731
    assert (np.array(old()) == np.array(new())).all() and (np.array(old()) == np.array(both())).all()
    n = args.repeats
    print(json.dumps(dict(size=list(r.image_res), repeats=n, host_convert_old_ms=_median_ms(old, n), host_convert_new_ms=_median_ms(new, n),
                          save_pack_and_convert_ms=_median_ms(both, n), fetch_image_ms=_median_ms(r.fetch_image, n), fetch_pixels_ms=_median_ms(r.fetch_pixels, n))), flush=True)
    r.close()


def run_trace(args):
    import ctypes
    r = make("cfg2", 1)
    r.accumulate(1)
    for _, arm in ARMS[1:]:
        r.set_pixels(arm[0], arm[1], seed=1, animate=True)
        for _ in range(40):
            r._lib.de_render_to_pixels(r._h, ctypes.byref(ctypes.c_void_p()))
        r.synchronize()
    print(json.dumps(dict(size=list(r.image_res), conversions_per_arm=40, order=[n for n, _ in ARMS[1:]])), flush=True)
    r.close()


def run_stats(args):
    """Per *kernel_trace.csv under the directory: pixels_pack_kernel's durations per arm (40 launches each, in ARMS' order, the first four of each dropped
    as warm-up) and display_kernel's."""
    for path in sorted(glob.glob(os.path.join(args.stats, "**", "*kernel_trace.csv"), recursive=True)):
        rows = {}
        for row in sorted(csv.DictReader(open(path)), key=lambda q: int(q["Start_Timestamp"])):
            k = row["Kernel_Name"].split("(")[0].replace("void ", "")
            if "pixels_pack_kernel" in k or "display_kernel" in k:
                rows.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3)
        print(os.path.relpath(path, args.stats))
        for k, us in sorted(rows.items()):
            groups = [(n, us[40 * i + 4:40 * (i + 1)]) for i, (n, _) in enumerate(ARMS[1:])] if "pixels_pack" in k and len(us) == 160 else [("all", us[4:])]
            for n, g in groups:
                print("  %-28s %-16s calls %4d  median %7.2f us  min %7.2f us  max %7.2f us" % (k, n, len(g), float(np.median(g)), float(np.min(g)), float(np.max(g))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--float-only", action="store_true")
    ap.add_argument("--save", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--stats", metavar="DIR")
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if args.loop:
        run_loop(args)
    if args.save:
        run_save(args)
    if args.trace:
        run_trace(args)
    if args.stats:
        run_stats(args)


if __name__ == "__main__":
    main()
