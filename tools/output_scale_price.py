"""Price of the output scaling (include/digital_earth_output_scale.h) -> profiles/output_scale.md.

    python tools/output_scale_price.py --passes             # the two passes per filter, 3840x2160 -> 1920x1080 and 960x544 -> 1920x1080
    python tools/output_scale_price.py --split              # each pass of 3840x2160 -> 1920x1080 on its own
    python tools/output_scale_price.py --loop [--unscaled-only]      # ms per frame of the pipelined pixel loop at 3840x2160 (--frames 60 --warmup 10 --repeats 5)

--passes: BASELINE cfg2's view rendered once at the source size; then the display chain alone is run --calls times back to back on the device
(de_render_to_image: nothing comes to the host) inside a host clock that ends in a device synchronise, with the stage off — display_kernel alone, the
yardstick — and on with each filter.  The difference per call is the stage: both passes, or the one pass of an axis pair.  The runs alternate inside
every repeat; each arm reports the median, minimum and maximum of its repeats, and the bytes the two passes must move (read + write of each) over the
difference.
--split: the same measurement with one axis a copy, so that one pass runs: 3840x2160 -> 3840x1080 is exactly the pass along v of the 4K case, and
3840x1080 -> 1920x1080 exactly its pass along u; each with the bytes that pass reads and writes over its time.
--loop: accumulate(1) + fetch_pixels(copy=False, lag=2) per frame at 3840x2160, RGBA8: unscaled (33 MB per frame over the link) against scaled to
1920x1080 with each filter (8 MB).  --unscaled-only uses nothing this feature added, so a copy of this file in the tools/ of a checkout of the parent
commit gives the comparison on the same machine; its spread over the repeats is the margin.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

FILTERS = ("box", "triangle", "mitchell", "lanczos3")


def make(size):
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd.earth_viewer import load_config
    from adaptive_price import VIEWS
    v = VIEWS["cfg2"]
    r = Renderer(size, (0, 1, 0), texture_source="synthetic", texture_quality=2, cloud_heavy=v["cloud_heavy"], seed=0)
    if v["preset"]:
        load_config(os.path.join(ROOT, "digital_earth_amd", "data", "configs", v["preset"])).apply(r)
    if v["crf_name"]:
        r.set_crf(r.crf_names.index(v["crf_name"]))
    r.copy_textures()
    return r


def _stats(v):
    return dict(median=round(float(np.median(v)), 2), min=round(float(np.min(v)), 2), max=round(float(np.max(v)), 2))


def _displays(r, calls):
    for _ in range(8):
        r.render_to_image_device()
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        r.render_to_image_device()
    r.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls


def run_passes(args):
    for src, dst in (((3840, 2160), (1920, 1080)), ((960, 544), (1920, 1080))):
        r = make(src)
        r.accumulate(1)
        r.synchronize()
        arms = [None] + list(FILTERS)
        us = {a: [] for a in arms}
        for _ in range(args.repeats):
            for a in arms:
                if a is None:
                    r.set_output_scale(on=False)
                else:
                    r.set_output_scale(dst, a)
                us[a].append(_displays(r, args.calls))
        r.set_output_scale(on=False)
        (W, H), (ow, oh) = src, dst
        moved = 12 * (W * H + W * oh) + 12 * (W * oh + ow * oh)      # pass along v reads the image and writes the intermediate; pass along u reads that and writes the output
        base = float(np.median(us[None]))
        print(json.dumps(dict(source=list(src), output=list(dst), calls=args.calls, repeats=args.repeats, display_only_us=_stats(us[None]))), flush=True)
        for a in FILTERS:
            stage = float(np.median(us[a])) - base
            taps = [int(r.debug_output_scale_weights(n, m, a)[1].shape[1]) for n, m in ((H, oh), (W, ow))]
            print(json.dumps(dict(source=list(src), output=list(dst), filter=a, taps_v_u=taps, display_and_scale_us=_stats(us[a]), stage_us=round(stage, 2),
                                  bytes_moved=moved, achieved_GBps=round(moved / stage / 1e3, 1) if stage > 0 else None)), flush=True)
        r.close()


def run_split(args):
    for name, src, dst in (("along v", (3840, 2160), (3840, 1080)), ("along u", (3840, 1080), (1920, 1080))):
        r = make(src)
        r.accumulate(1)
        r.synchronize()
        arms = [None] + list(FILTERS)
        us = {a: [] for a in arms}
        for _ in range(args.repeats):
            for a in arms:
                if a is None:
                    r.set_output_scale(on=False)
                else:
                    r.set_output_scale(dst, a)
                us[a].append(_displays(r, args.calls))
        r.set_output_scale(on=False)
        moved = 12 * (src[0] * src[1] + dst[0] * dst[1])
        base = float(np.median(us[None]))
        for a in FILTERS:
            stage = float(np.median(us[a])) - base
            print(json.dumps(dict(pass_=name, source=list(src), output=list(dst), filter=a, display_only_us=_stats(us[None]), pass_us=round(stage, 2), bytes_moved=moved,
                                  achieved_GBps=round(moved / stage / 1e3, 1) if stage > 0 else None)), flush=True)
        r.close()


def one_loop(r, arm, warmup, frames):
    if arm is not None:
        r.set_output_scale((1920, 1080), arm)
    r.reset_framebuffer()
    for _ in range(warmup):
        r.accumulate(1)
        r.fetch_pixels(copy=False, lag=2)
    r.fetch_pending(copy=False, pixels=True)
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        r.accumulate(1)
        r.fetch_pixels(copy=False, lag=2)
    r.fetch_pending(copy=False, pixels=True)
    r.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / frames
    if arm is not None:
        r.set_output_scale(on=False)
    return ms


def run_loop(args):
    r = make((3840, 2160))
    arms = [None] if args.unscaled_only else [None] + list(FILTERS)
    ms = {a: [] for a in arms}
    for _ in range(args.repeats):
        for a in arms:
            ms[a].append(one_loop(r, a, args.warmup, args.frames))
    for a, v in ms.items():
        print(json.dumps(dict(arm="unscaled 3840x2160 RGBA8" if a is None else "scaled to 1920x1080 RGBA8, %s" % a, lag=2, frames=args.frames, repeats=args.repeats,
                              ms_per_frame_median=round(float(np.median(v)), 3), ms_min=round(float(np.min(v)), 3), ms_max=round(float(np.max(v)), 3))), flush=True)
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", action="store_true")
    ap.add_argument("--split", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--unscaled-only", action="store_true")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if args.passes:
        run_passes(args)
    if args.split:
        run_split(args)
    if args.loop:
        run_loop(args)


if __name__ == "__main__":
    main()
