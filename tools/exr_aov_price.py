"""What the EXR output's AOV channels cost (profiles/exr_aovs.md): at 1920x1080, HALF + ZIP, the denoiser on from the reset, 4 samples per pixel,
    python tools/exr_aov_price.py [--repeats 3] [--calls 20]
prints, as medians with minimum and maximum over the repeats (the arms alternate inside every repeat, the first pass is dropped):
  the conversion on the device (render_to_exr + synchronize) with every AOV on beside the mask-0 conversion of the same frame;
  the pipelined loop fetch_exr(lag=2) with every AOV on beside the loop it replaces, fetch_guides() + fetch_hdr() + the host's division,
  orientation and conversion to the planes' types (no host deflate);
  the file's size and the share of raw blocks.
The time of exr_aov_layout_kernel alone is a profiler's: rocprofv3 --kernel-trace --stats -- python tools/exr_aov_price.py --calls 5 --repeats 1"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    a = ap.parse_args()
    from digital_earth_amd import exr
    from digital_earth_amd.renderer import Renderer
    W, H = a.size
    r = Renderer((W, H), (0, 1, 0), texture_source="synthetic", texture_size=(1024, 512))
    r.copy_textures()
    r.set_denoise(True)
    r.reset_framebuffer()
    r.accumulate(4)
    r.synchronize()

    def convert():
        t = time.perf_counter()
        for _ in range(a.calls):
            r.render_to_exr()
        r.synchronize()
        return (time.perf_counter() - t) / a.calls * 1e3

    def ring():
        t = time.perf_counter()
        for _ in range(a.calls):
            r.fetch_exr(copy=False, lag=2)
        r.fetch_pending_exr(copy=False)
        return (time.perf_counter() - t) / a.calls * 1e3

    def host():
        t = time.perf_counter()
        for _ in range(a.calls):
            g = r.fetch_guides()
            s1 = r.fetch_hdr()
            mean = np.ascontiguousarray((s1 / np.float32(r.current_spp))[:, ::-1].transpose(1, 0, 2))
            g = np.ascontiguousarray(g[:, ::-1].transpose(1, 0, 2))
            planes = [np.clip(mean, -65504, 65504).astype(np.float16), g[..., 1].copy(), np.clip(g[..., [0, 2, 3, 4, 5, 6, 7, 8]], -65504, 65504).astype(np.float16)]
            del planes
        return (time.perf_counter() - t) / a.calls * 1e3

    arms = {"convert, mask 0": (convert, ()), "convert, all": (convert, "all"), "fetch_exr(lag=2), all": (ring, "all"), "fetch_guides + fetch_hdr + host": (host, ())}
    times = {k: [] for k in arms}
    for rep in range(a.repeats + 1):
        for name, (fn, aovs) in arms.items():
            r.set_exr(aovs=aovs)
            ms = fn()
            if rep:
                times[name].append(ms)
    for name, v in times.items():
        print("%-36s %8.3f ms  (min %.3f, max %.3f, %d x %d calls)" % (name, statistics.median(v), min(v), max(v), len(v), a.calls))
    for aovs in ((), "all"):
        r.set_exr(aovs=aovs)
        data = r.fetch_exr()
        blocks = exr.read(data)[1]["blocks"]
        print("file, aovs=%r: %d bytes of capacity %d, %d of %d blocks raw" % (aovs, len(data), r.exr()["capacity"], sum(b["raw"] for b in blocks), len(blocks)))
    r.close()


if __name__ == "__main__":
    main()
