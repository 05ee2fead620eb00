#!/usr/bin/env python3
"""What the HDR display output costs (profiles/hdr_output.md): the display launch with the stage off (display_kernel) and on
(hdr_display_kernel, per transfer), and the pack behind it (hdr_pack_kernel, per format), at one size on one GPU in ONE process.

    python tools/hdr_output_price.py [--size 1920 1080] [--reps 5000] [--rounds 5]

Method: a frame of 2 spp is rendered once; then every variant is timed as `reps` back-to-back calls between two host clock reads with a
synchronize before each read (launch overhead amortised over the queue; nothing else runs on the context; 5000 calls of 30 - 55 us are a window of
0.15 - 0.3 s), `rounds` times, the variants interleaved within a round so that clock drift and neighbours hit all of them alike.  Reported: the
median over rounds of the per-call time, and min - max.  The display variants are whole de_render_to_image calls (setup check, the launch, an event
record), the pack variants whole de_render_to_hdr_pixels calls under PQ; the last lines print, per pack variant, its median minus the PQ display's
median: what the pack adds to a call.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/hdr_output_price.py --trace
    python tools/hdr_output_price.py --summarize DIR

KERNEL times, in a run of their own: --trace runs TRACE_CALLS calls per arm in the order of the table below and times nothing; --summarize reads the
trace, cuts each kernel's launches into the arms by that order, drops the first four of an arm and prints median, minimum and maximum per arm."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


TRACE_CALLS = 40


def device_name():
    """What the runtime calls the GPU the numbers come from (the profile quotes it)."""
    try:
        import torch
        p = torch.cuda.get_device_properties(0)
        return "%s, %s, %d CUs" % (p.name, getattr(p, "gcnArchName", "?"), p.multi_processor_count)
    except Exception as e:      # the tool measures without torch just as well
        return "unknown (%s)" % type(e).__name__


def summarize(directory):
    import csv
    import glob
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    by = {}
    for r in rows:
        for key in ("hdr_display_kernel", "hdr_pack_kernel", "display_kernel"):
            if key in r["Kernel_Name"]:
                by.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
                break
    arms = {"display_kernel": ["stage off"], "hdr_display_kernel": ["linear", "pq", "hlg", "pq (ahead of the pack arms, 4 x %d launches)" % TRACE_CALLS],
            "hdr_pack_kernel": ["rgb10a2 truncate", "rgb10a2 dither", "rgb16 truncate", "rgb16 dither"]}
    for key, names in arms.items():
        t = by.get(key, [])
        t = t[-(TRACE_CALLS * (len(names) + (3 if key == "hdr_display_kernel" else 0))):]      # the launches of the timed frame's arms: not the warm-up display
        for k, name in enumerate(names):
            arm = t[k * TRACE_CALLS:(k + 1) * TRACE_CALLS] if not name.startswith("pq (") else t[3 * TRACE_CALLS:]
            arm = arm[4:]
            if arm:
                print("%-20s %-48s %4d launches  median %7.2f us  min %7.2f  max %7.2f" % (key, name, len(arm), statistics.median(arm), min(arm), max(arm)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--summarize", default=None)
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
    ap.add_argument("--reps", type=int, default=5000)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    from digital_earth_amd.renderer import Renderer
    r = Renderer(tuple(a.size), (0, 1, 0), texture_source="synthetic", texture_size=(2048, 1024))
    r.copy_textures()
    r.accumulate(2)
    r.synchronize()

    def timed(call):
        for _ in range(20):
            call()
        r.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            call()
        r.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e6

    variants = [("display_kernel (stage off)", None, r.render_to_image_device)]
    for transfer in ("linear", "pq", "hlg"):
        variants.append(("hdr_display_kernel %s" % transfer, dict(transfer=transfer), r.render_to_image_device))
    for fmt in ("rgb10a2", "rgb16"):
        for mode in ("truncate", "dither"):
            variants.append(("display pq + hdr_pack_kernel %s %s" % (fmt, mode), dict(transfer="pq", pixel_format=fmt, mode=mode), r.render_to_hdr_pixels_device))
    if a.trace:
        print("device:", device_name())
        for name, setting, call in variants:
            if setting is None:
                r.set_hdr_output(False)
            else:
                r.set_hdr_output(True, **setting)
            for _ in range(TRACE_CALLS):
                call()
            r.synchronize()
        r.close()
        return
    times = {name: [] for name, _, _ in variants}
    for _ in range(a.rounds):
        for name, setting, call in variants:
            if setting is None:
                r.set_hdr_output(False)
            else:
                r.set_hdr_output(True, **setting)
            times[name].append(timed(call))
    out = {"size": list(a.size), "reps": a.reps, "rounds": a.rounds, "device": device_name(), "us_per_call": {}}
    for name, ts in times.items():
        out["us_per_call"][name] = {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "max": round(max(ts), 2)}
        print("%-52s median %8.2f us   (%.2f - %.2f)" % (name, statistics.median(ts), min(ts), max(ts)))
    base = out["us_per_call"]["hdr_display_kernel pq"]["median"]
    out["pack_adds_us"] = {}
    for name in times:
        if "hdr_pack_kernel" in name:
            out["pack_adds_us"][name] = round(out["us_per_call"][name]["median"] - base, 2)
            print("%-52s adds   %8.2f us to the PQ display's call" % (name, out["pack_adds_us"][name]))
    print(json.dumps(out))
    r.close()


if __name__ == "__main__":
    main()
