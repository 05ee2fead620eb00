"""Price of the denoiser (include/digital_earth_denoise.h) on the four BASELINE views -> profiles/denoise.md.

    python tools/denoise_price.py --time            # wall time of the guides and of the filter at each view's BASELINE size
    python tools/denoise_price.py --quality --scale 4

--time: per view at its BASELINE size, the host wall time (after a synchronize, mean of --reps calls) of a denoised display minus a plain one (the filter:
prep + levels), and of the first denoised display of a frame minus a later one (the guides).  Device times per kernel come from a separate
`rocprofv3 --kernel-trace --stats` run of this script.
--quality: per view at 1/scale of its size, relative L2 of the displayed image and of the HDR mean, raw and denoised, at 1 / 4 / 16 / 64 spp, against a
frame of another seed at 4 x the largest spp; and the raw spp whose error (fitted as a / sqrt(n)) equals the denoised 16-spp frame's.
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

from adaptive_price import VIEWS, make, rel_l2  # noqa: E402


def accumulate(r, spp):
    left = spp
    while left > 0:
        n = min(left, 64)
        r.accumulate(n)
        left -= n


def timed(fn, reps):
    fn()
    s = 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        s += time.perf_counter() - t0
    return s / reps * 1e3


def run_time(args):
    for name in args.configs:
        r = make(name, 1)
        r.reset_framebuffer()
        accumulate(r, 4)
        r.synchronize()
        plain = timed(lambda: r.fetch_image(), args.reps)
        r.set_denoise(True)
        den = timed(lambda: r.fetch_image(), args.reps)

        def first():
            r.reset_framebuffer()
            r.set_current_spp(4)      # an empty frame of 4 spp: the display runs, the guides are recomputed after the reset
            r.fetch_image()
        first_ms = timed(first, args.reps)

        def later():
            r.set_current_spp(4)
            r.fetch_image()
        later_ms = timed(later, args.reps)
        print(json.dumps(dict(view=name, size=list(r.image_res), plain_display_ms=plain, denoised_display_ms=den, filter_ms=den - plain,
                              guides_ms=first_ms - later_ms)), flush=True)
        r.close()


def run_quality(args):
    steps = (1, 4, 16, 64)
    for name in args.configs:
        r = make(name, args.scale)
        r.seed = 1000
        r.reset_framebuffer()
        accumulate(r, 4 * steps[-1])
        ref_img, ref_hdr = r.fetch_image(), r.fetch_hdr() / (4 * steps[-1])
        r.seed = 0
        rows = []
        for spp in steps:
            r.set_denoise(True)
            r.reset_framebuffer()
            accumulate(r, spp)
            den_img, den_hdr = r.fetch_image(), r.fetch_denoised_hdr()
            r.set_denoise(False)
            raw_img, raw_hdr = r.fetch_image(), r.fetch_hdr() / spp
            rows.append(dict(spp=spp, image_raw=rel_l2(raw_img, ref_img), image_den=rel_l2(den_img, ref_img),
                             hdr_raw=rel_l2(raw_hdr, ref_hdr), hdr_den=rel_l2(den_hdr, ref_hdr)))
        # raw error ~ a / sqrt(n) (least squares in log space over the four counts); the n at which it equals the denoised 16-spp error
        n = np.array([x["spp"] for x in rows], np.float64)
        match = {}
        for key in ("image", "hdr"):
            e = np.array([x[key + "_raw"] for x in rows])
            loga = float(np.mean(np.log(e) + 0.5 * np.log(n)))
            target = rows[2][key + "_den"]
            match[key] = float(np.exp(2.0 * (loga - np.log(target))))
        print(json.dumps(dict(view=name, size=list(r.image_res), reference_spp=4 * steps[-1], rows=rows, raw_spp_matching_denoised_16=match)), flush=True)
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=list(VIEWS), choices=list(VIEWS))
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.time:
        run_time(args)
    if args.quality:
        run_quality(args)


if __name__ == "__main__":
    main()
