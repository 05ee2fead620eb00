"""What the PNG output costs and how long its files are (include/digital_earth_png.h; the tables of profiles/png.md).

    python tools/png_price.py --encode [--repeats 5] [--n 100]     de_render_to_png per source {rgb8, rgba8, rgb16} and chunk size {4096, 8192, 16384,
                                                                   32768, 65535} against de_render_to_image on one 1920x1080 context, and each
                                                                   file's length
    python tools/png_price.py --length [--spp 16]                  the BASELINE cameras at 1920x1080: the GPU's file per chunk size against the same
                                                                   filtered bytes through zlib level 6 (what the host writers use) and Z_RLE
    python tools/png_price.py --loop [--repeats 3] [--frames 60]   the recording loop (accumulate(1), fetch_png(lag=1)) against what a caller had
                                                                   before: the pipelined fetch_pixels loop plus the host encode save() performs

Host clock around work that ends in a device synchronise; the arms alternate inside every repeat; every arm is warmed up first (the first pass over
the arms is dropped).  Prints one JSON line per mode."""
import argparse
import io
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from adaptive_price import make  # noqa: E402

W, H = 1920, 1080
CHUNKS = (4096, 8192, 16384, 32768, 65535)
SOURCES = ("rgb8", "rgba8", "rgb16")


def _summary(xs):
    return dict(median=round(statistics.median(xs), 3), min=round(min(xs), 3), max=round(max(xs), 3))


def _renderer(name="cfg2", spp=4):
    r = make(name, 2 if name == "cfg4" else 1)      # every BASELINE view at 1920 x 1080 (cfg4 is a 4K view: halved)
    assert tuple(r.image_res) == (W, H)
    r.accumulate(spp)
    return r


def _source(r, source):
    if source == "rgb16":
        r.set_hdr_output(True, pixel_format="rgb16", mode="round")
    else:
        r.set_hdr_output(False)
        r.set_pixels(3 if source == "rgb8" else 4, "round")
    return "hdr_pixels" if source == "rgb16" else "pixels"


def encode(args):
    r = _renderer()
    times, sizes = {}, {}
    arms = [("render_to_image " + s, s, None) for s in SOURCES] + [("render_to_png %s chunk %d" % (s, c), s, c) for s in SOURCES for c in CHUNKS]
    for rep in range(args.repeats + 1):
        for name, source, chunk in arms:
            src = _source(r, source)
            if chunk:
                r.set_png(source=src, chunk_bytes=chunk)
                sizes[name] = len(r.fetch_png())
            fn = r.render_to_png if chunk else r.render_to_image_device
            fn()
            r.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.n):
                fn()
            r.synchronize()
            if rep:
                times.setdefault(name, []).append((time.perf_counter() - t0) / args.n * 1e6)
    print(json.dumps(dict(what="microseconds per call back to back, the display transform included; bytes per file", size=[W, H], n=args.n,
                          repeats=args.repeats, arms={k: _summary(x) for k, x in times.items()}, bytes=sizes)), flush=True)
    r.close()


def length(args):
    import png_ref
    out = {}
    for name in ("cfg2", "cfg3", "cfg4", "cfg5"):
        r = _renderer(name, args.spp)
        r.set_pixels(3, "round")
        S = png_ref.filtered_stream(r.fetch_pixels()).tobytes()
        row = dict(filtered=len(S), zlib6=len(zlib.compress(S, 6)))
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        row["zlib_rle"] = len(c.compress(S) + c.flush())
        for chunk in CHUNKS:
            r.set_png(chunk_bytes=chunk)
            row["gpu_%d" % chunk] = len(r.fetch_png()) - 33 - 12 - 12      # the deflate stream and its IDAT framing: without signature, IHDR, IEND
        out[name] = row
        r.close()
    print(json.dumps(dict(what="bytes: the filtered stream of the RGB8 frame, zlib level 6 and Z_RLE on it, the GPU's IDATs per chunk size", size=[W, H],
                          spp=args.spp, views=out)), flush=True)


def loop(args):
    from PIL import Image
    r = _renderer()
    r.set_pixels(3, "round")
    r.set_png()
    arms = ("png on the GPU", "pixels rgb8 + host encode", "pixels rgb8 alone")
    times, nbytes = {name: [] for name in arms}, {}
    for rep in range(args.repeats + 1):
        for name in arms:
            gpu = name == arms[0]
            fetch = (lambda: r.fetch_png(copy=False, lag=1)) if gpu else (lambda: r.fetch_pixels(copy=False, lag=1))
            drain = (lambda: r.fetch_pending_png(copy=False)) if gpu else (lambda: r.fetch_pending(copy=False, pixels=True))
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
                    Image.fromarray(got).save(buf, "PNG")      # what EarthViewer.save does with the pixels without set_png
                    nbytes[name] = buf.tell()
            del got
            drain()
            r.synchronize()
            if rep:
                times[name].append((time.perf_counter() - t0) / args.frames * 1e3)
    print(json.dumps(dict(what="ms per frame: accumulate(1) + pipelined fetch (lag 1), zero-copy view", size=[W, H], frames=args.frames,
                          repeats=args.repeats, arms={k: _summary(x) for k, x in times.items()}, bytes_per_frame=nbytes)), flush=True)
    r.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--encode", action="store_true")
    ap.add_argument("--length", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--spp", type=int, default=16)
    a = ap.parse_args()
    if a.encode:
        encode(a)
    if a.length:
        length(a)
    if a.loop:
        loop(a)
