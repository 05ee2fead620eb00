"""What the video frame output costs (include/digital_earth_video.h; the tables of profiles/video_output.md).

    python tools/video_price.py --calls [--repeats 5] [--n 300]      de_render_to_video against de_render_to_pixels (RGBA8) on one 1920x1080 context
    python tools/video_price.py --loop  [--repeats 3] [--frames 100] the recording loop (accumulate(1), fetch_video(lag=1)) against the pixel loop
    python tools/video_price.py --trace                              conversions left on the device, for `rocprofv3 --kernel-trace --stats -- python ...`

Host clock around work that ends in a device synchronise; the arms alternate inside every repeat; every arm is warmed up first (the first pass over
the arms is dropped).  Prints one JSON line per mode."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from adaptive_price import make  # noqa: E402

W, H = 1920, 1080
VIDEO_ARMS = (("nv12", "round"), ("i420", "round"), ("p010", "round"), ("i010", "round"), ("nv12", "dither"), ("i010", "dither"))


def _summary(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def _renderer():
    r = make("cfg2", 1)      # BASELINE cfg2's view at 1920 x 1080, as tools/pixels_price.py
    assert tuple(r.image_res) == (W, H)
    r.accumulate(4)
    r.set_pixels(4, "truncate")
    return r


def _to_pixels(r):
    r._lib.de_render_to_pixels(r._h, ctypes.byref(ctypes.c_void_p()))


def calls(args):
    r = _renderer()
    arms = [("render_to_image", None, r.render_to_image_device), ("render_to_pixels rgba8 truncate", None, lambda: _to_pixels(r))]
    arms += [("render_to_video %s %s" % a, a, r.render_to_video) for a in VIDEO_ARMS]
    times = {name: [] for name, _, _ in arms}
    for rep in range(args.repeats + 1):
        for name, setting, fn in arms:
            if setting:
                r.set_video(setting[0], mode=setting[1], siting="left")
            fn()
            r.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.n):
                fn()
            r.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) / args.n * 1e6)
    print(json.dumps(dict(what="microseconds per call back to back, the display transform included", size=[W, H], n=args.n, repeats=args.repeats,
                          arms={k: _summary(x) for k, x in times.items()})), flush=True)
    r.close()


def loop(args):
    r = _renderer()
    arms = [("pixels rgba8", None), ("video nv12", "nv12"), ("video i420", "i420"), ("video i010", "i010")]
    times = {name: [] for name, _ in arms}
    nbytes = {}
    for rep in range(args.repeats + 1):
        for name, fmt in arms:
            if fmt:
                r.set_video(fmt)
            # what EarthViewer.frame(video=True / pixels=True, pipelined=1) runs per iteration
            fetch = (lambda: r.fetch_video(copy=False, lag=1)) if fmt else (lambda: r.fetch_pixels(copy=False, lag=1))
            drain = (lambda: r.fetch_pending(copy=False, video=True)) if fmt else (lambda: r.fetch_pending(copy=False, pixels=True))
            r.reset_framebuffer()
            for _ in range(args.warmup):
                r.accumulate(1)
                fetch()
            drain()
            r.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.frames):
                r.accumulate(1)
                got = fetch()
            nbytes[name] = int(np.asarray(got).nbytes)
            del got
            drain()
            r.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    print(json.dumps(dict(what="ms per frame: accumulate(1) + pipelined fetch (lag 1), zero-copy view", size=[W, H], frames=args.frames, repeats=args.repeats,
                          arms={k: _summary(x) for k, x in times.items()}, bytes_per_frame=nbytes)), flush=True)
    r.close()


def trace(args):
    r = _renderer()
    for _ in range(40):
        _to_pixels(r)
    for fmt, mode in VIDEO_ARMS:
        r.set_video(fmt, mode=mode)
        for _ in range(40):
            r.render_to_video()
    r.synchronize()
    print(json.dumps(dict(what="40 launches of pixels_pack_kernel, then 40 of videoframe_pack_kernel per arm", arms=[list(a) for a in VIDEO_ARMS])), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if a.calls:
        calls(a)
    if a.loop:
        loop(a)
    if a.trace:
        trace(a)
