"""What the JPEG output costs (include/digital_earth_jpeg.h; the tables of profiles/jpeg.md).

    python tools/jpeg_price.py --restart [--repeats 5] [--n 200]     de_render_to_jpeg per restart interval {1, 2, 4, 8, 16, one MCU row} against
                                                                     de_render_to_image on one 1920x1080 context, and each stream's length
    python tools/jpeg_price.py --loop [--repeats 3] [--frames 100]   the recording loop (accumulate(1), fetch_jpeg(lag=1)) against what a caller had before:
                                                                     the pipelined fetch_pixels loop plus Pillow's encode of that frame, same quality, 4:2:0
    python tools/jpeg_price.py --trace                               conversions left on the device, for `rocprofv3 --kernel-trace --stats -- python ...`

Host clock around work that ends in a device synchronise; the arms alternate inside every repeat; every arm is warmed up first (the first pass over
the arms is dropped).  Prints one JSON line per mode."""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from adaptive_price import make  # noqa: E402

W, H = 1920, 1080
ROW = (W + 15) // 16
RESTARTS = (1, 2, 4, 8, 16, ROW)
QUALITY = 90


def _summary(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def _renderer():
    r = make("cfg2", 1)      # BASELINE cfg2's view at 1920 x 1080, as tools/video_price.py
    assert tuple(r.image_res) == (W, H)
    r.accumulate(4)
    return r


def restart(args):
    r = _renderer()
    arms = [("render_to_image", None)] + [("render_to_jpeg restart %d" % n, n) for n in RESTARTS]
    times = {name: [] for name, _ in arms}
    sizes = {}
    for rep in range(args.repeats + 1):
        for name, n in arms:
            if n:
                r.set_jpeg(QUALITY, n)
                sizes[name] = len(r.fetch_jpeg())
            fn = r.render_to_jpeg if n else r.render_to_image_device
            fn()
            r.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.n):
                fn()
            r.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) / args.n * 1e6)
    print(json.dumps(dict(what="microseconds per call back to back, the display transform included; bytes per stream", size=[W, H], quality=QUALITY, n=args.n,
                          repeats=args.repeats, arms={k: _summary(x) for k, x in times.items()}, bytes=sizes)), flush=True)
    r.close()


def loop(args):
    from PIL import Image
    r = _renderer()
    r.set_pixels(3, "round")
    r.set_jpeg(QUALITY)
    arms = ("jpeg on the GPU", "pixels rgb8 + Pillow encode", "pixels rgb8 alone")
    times = {name: [] for name in arms}
    nbytes = {}
    for rep in range(args.repeats + 1):
        for name in arms:
            gpu = name == arms[0]
            fetch = (lambda: r.fetch_jpeg(copy=False, lag=1)) if gpu else (lambda: r.fetch_pixels(copy=False, lag=1))
            drain = (lambda: r.fetch_pending_jpeg(copy=False)) if gpu else (lambda: r.fetch_pending(copy=False, pixels=True))
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
                if got is None:
                    continue
                if gpu:
                    nbytes[name] = len(got)
                elif name == arms[1]:
                    buf = io.BytesIO()
                    Image.fromarray(got).save(buf, "JPEG", quality=QUALITY, subsampling=2)      # 4:2:0, the typical tables, one thread
                    nbytes[name] = buf.tell()
            del got
            drain()
            r.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    print(json.dumps(dict(what="ms per frame: accumulate(1) + pipelined fetch (lag 1), zero-copy view", size=[W, H], quality=QUALITY, frames=args.frames,
                          repeats=args.repeats, arms={k: _summary(x) for k, x in times.items()}, bytes_per_frame=nbytes)), flush=True)
    r.close()


def trace(args):
    r = _renderer()
    r.set_video("i420", "bt601", "full", "center")
    for _ in range(40):
        r.render_to_video()
    for n in (8, ROW):
        r.set_jpeg(QUALITY, n)
        for _ in range(40):
            r.render_to_jpeg()
    r.synchronize()
    print(json.dumps(dict(what="40 launches of videoframe_pack_kernel alone, then 40 conversions at restart 8 and 40 at one MCU row")), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--restart", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if a.restart:
        restart(a)
    if a.loop:
        loop(a)
    if a.trace:
        trace(a)
