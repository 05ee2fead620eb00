#!/usr/bin/env python3
"""bench.py — Msamples/s of the spectral path-tracing hot path on N MI355X (BASELINE.json metric).

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

One "step" = one frame of the workload: reset_framebuffer, accumulate(spp) on this rank's 8x8 tiles, (N > 1) one
RCCL sum-reduce of the HDR buffer to rank 0, and the display transform on rank 0.  Textures and LUTs are resident
in HBM before the timed region (the reference uploads them once, renderer.py:136-145).  The frame is FIXED and split
over the ranks (tile partition), so scaling is "strong".  Rank 0 prints ONE JSON line.

Workload (BASELINE.json configs[1]): 1920x1080, 64 spp, full spectral Rayleigh+Mie+O3+clouds, quality-2 maps
(21600x10800 / 16200x8100, synthetic stand-ins: the reference ships no maps), default camera and sun.

`--config cfg2|cfg3|cfg4|cfg5` runs any BASELINE config by name (size, sample count, the reference's camera preset, cloud-heavy maps, progressive interval;
the line's `metric` names it).  A plain run sets up, warms up, times --steps frames and prints the line (`--dump-outputs DIR`: the last timed frame as .npy
files first).  `--full` adds everything else, after the timed region: the single-frame, roofline and VALU figures (untimed frames of their own), with N > 1
the other launch setting (`alt`), the parity check of the assembled frame and the in-library communicator's frame, and on the default 1-GPU run
`other_configs` (cfg3 / cfg4 / cfg5 for two steps each, the frame at the config's full sample count checked against the oracle on sparse tiles),
`cpu_baseline` (the oracle on a bounded sample, all host threads) and `parity` (the full-size frame against the oracle's at matched seed).  One-GPU experiments for the N-rank path: `--simulate-world N` (rank 0's share, no collective),
`--standin-collective COPIES` (a stand-in for the frame's collective where the reduce goes), `--cu-withhold n` (CUs per XCD left to the small kernels).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# before anything initialises HIP (torch included): enough hardware queues for the library's launch slots to run side by side
# (digital_earth_amd/_native.py sets the same default when it loads the library first)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")

HBM_PEAK_GBPS = 8000.0          # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md

# BASELINE.json `configs` by name (configs[0] — 256x256, 4 spp, one wavelength, flat Earth — is the reference's CPU-runnable case: a parity test,
# tests/test_gpu_parity.py, not a bench workload).  `--config NAME` sets size / spp / camera preset / map variant / progressive interval from this table
# and the line's `metric` names the config; the presets are the reference's own `config - *.txt` files (digital_earth_amd/data/configs, sha256-pinned).
# cfg5's camera-response curve is taken BY NAME: the preset's index 12 counts os.listdir order on the author's machine; the name is the one
# the executed reference resolved it to in the build container (tests/golden/ref_q2.npz: apollo_crf_name).
CONFIGS = {
    "cfg2": dict(index=1, width=1920, height=1080, spp=64, preset=None, cloud_heavy=False, progressive=0, crf_name=None),
    "cfg3": dict(index=2, width=1920, height=1080, spp=256, preset="config - florida.txt", cloud_heavy=False, progressive=0, crf_name=None),
    "cfg4": dict(index=3, width=3840, height=2160, spp=128, preset="config - sunset hurricane.txt", cloud_heavy=True, progressive=0, crf_name=None),
    "cfg5": dict(index=4, width=1920, height=1080, spp=1024, preset="config - Apollo 11.txt", cloud_heavy=False, progressive=128, crf_name="kaf2001CD.rf"),
}
# sparse-tile oracle check of a config at its FULL sample count: every `stride`-th 8x8 tile in raster order (spread over the whole frame), ~0.5 M paths on the host
SPARSE_CHECK = {"cfg2": (5, 251), "cfg3": (11, 997), "cfg4": (23, 2003), "cfg5": (41, 4051)}
# --dump-outputs writes at most this many bytes: cfg2's two whole frames (49.8 MB) fit, larger frames are sampled
DUMP_LIMIT_BYTES = 64 * 10**6


def metric_name(width, height, spp, preset, cloud_heavy, progressive):
    extra = ""
    if preset:
        extra += ", '%s'" % preset
    if cloud_heavy:
        extra += ", cloud-heavy maps"
    if progressive:
        extra += ", progressive every %d" % progressive
    return "Msamples/sec (%dx%d, %d spp%s) spectral path tracing" % (width, height, spp, extra)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None,
                    help="a BASELINE.json config by name: sets --width/--height/--spp/--preset/--cloud-heavy/--progressive (and cfg5's film curve) and the line's metric string; "
                         "default: cfg2 = BASELINE configs[1], the configuration the metric is quoted on")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="default 1-GPU cfg2 run: skip the short (2-step) legs of cfg3 / cfg4 / cfg5 that follow the timed region (`other_configs` in the line)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--tex-quality", type=int, default=2)
    ap.add_argument("--preset", default=None, help="camera preset file name under digital_earth_amd/data/configs")
    ap.add_argument("--cloud-heavy", action="store_true")
    ap.add_argument("--frames-in-flight", type=int, default=1,
                    help="independent frame contexts alternated step by step.  Default 1: since round 3 the library overlaps the "
                         "launches of ONE context itself (launch slots, de_accumulate in include/digital_earth.h); >1 is the round-2 scheme")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--simulate-world", type=int, default=0, help="1-GPU experiment: render only rank 0's share of an N-rank tile partition (no collective); not a bench line")
    ap.add_argument("--cpu-spp", type=int, default=8, help="upper bound on the spp of the bounded CPU-baseline sample (~15 s)")
    ap.add_argument("--integrator", choices=("path_tracer", "ray_marcher"), default="path_tracer",
                    help="ray_marcher = the reference's alternative integrator (pathtracer.py:471-685, SURVEY §8f-3); not the BASELINE metric")
    ap.add_argument("--tex-size", type=int, nargs=2, default=None, help="override the size of every synthetic map (tests)")
    ap.add_argument("--reduce", choices=("torch", "lib"), default=os.environ.get("DE_REDUCE", "torch"),
                    help="N > 1 collective: torch.distributed (default) or the library's own RCCL communicator (de_comm_init / de_reduce)")
    ap.add_argument("--split", choices=("tiles", "samples"), default=os.environ.get("DE_SPLIT", "tiles"),
                    help="N > 1 partition of the frame: 8x8 tiles dealt diagonally + sum-reduce (default, north_star), or sample indices dealt "
                         "round robin + rank-ordered gather-sum (SURVEY §8e's alternative; with --simulate-world: rank 0's share of either)")
    ap.add_argument("--progressive", type=int, default=0, metavar="K",
                    help="progressive frames (BASELINE cfg5, SURVEY §8e): out-of-place reduce + display every K spp instead of once per frame")
    ap.add_argument("--waves-per-cu", type=int, default=0,
                    help="render_kernel_v2 only (calls below 4096 paths, counting launches): resident waves per CU, 1..20.  The timed kernel, "
                         "render_kernel_v6, always runs two workgroups of 12 waves per CU and ignores this")
    ap.add_argument("--sync-frames", action="store_true",
                    help="wait for every frame before submitting the next (profiling: frames do not overlap in the trace)")
    ap.add_argument("--collective", choices=("reduce", "gather"), default="reduce",
                    help="N > 1, tile partition, --reduce torch: sum-reduce of the whole HDR buffer (default) or a gather of each rank's own pixels (1/N of the bytes; SURVEY §8e)")
    ap.add_argument("--serial-frames", action="store_true",
                    help="one launch at a time (launch slots = 1): the collective of frame k never waits behind frame k+1's persistent waves")
    ap.add_argument("--standin-collective", type=int, default=-1, metavar="COPIES",
                    help="1-GPU experiment (with --simulate-world N): enqueue a stand-in for the frame's collective where the reduce goes — one streaming kernel over the HDR buffer "
                         "+ COPIES device-to-device copies of it (7 = the ingress of an 8-rank gather) — and report its queue-to-finish latency (`standin_collective`)")
    ap.add_argument("--cu-withhold", type=int, default=0, help="CUs per XCD withheld from the render launches' streams (de_tuning.v6_cu_withhold)")
    ap.add_argument("--dump-hdr", default=None, help="rank 0: save the assembled HDR frame of the LAST step as .npy (tests)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0, after the timed steps: what the last step handed its caller, as DIR/hdr.npy (the assembled HDR frame) and DIR/image.npy "
                         "(its display transform), float32 (W, H, 3); above %d MB in all, the same fixed seeded sample of pixels of both, (n, 3)" % (DUMP_LIMIT_BYTES // 10**6))
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything besides the headline figure (module docstring); without it the run only sets up, warms up, "
                         "times --steps frames and prints the line")
    ap.add_argument("--check-spp", type=int, default=2, help="N > 1: spp of the untimed parity check of the assembled frame against a 1-rank render on rank 0 (0 = skip)")
    args = ap.parse_args()
    args.crf_name = None
    args.config_name = None
    if args.config:
        c = CONFIGS[args.config]
        args.width, args.height, args.spp, args.preset = c["width"], c["height"], c["spp"], c["preset"]
        args.cloud_heavy, args.progressive, args.crf_name = c["cloud_heavy"], c["progressive"], c["crf_name"]
        args.tex_quality = 2
        args.config_name = args.config
    else:
        # flags that happen to spell a BASELINE config are named as one; anything else gets a metric string that says what ran
        for name, c in CONFIGS.items():
            if (args.width, args.height, args.spp, args.preset, bool(args.cloud_heavy), args.progressive) == (c["width"], c["height"], c["spp"], c["preset"], c["cloud_heavy"], c["progressive"]) \
                    and args.tex_quality == 2 and not args.tex_size and c["crf_name"] is None:
                args.config_name = name
    return args


def apply_preset(r, name, crf_name=None):
    from digital_earth_amd.earth_viewer import load_config
    cfg = load_config(os.path.join(ROOT, "digital_earth_amd", "data", "configs", name))
    cfg.apply(r)
    if crf_name:
        r.set_crf(r.crf_names.index(crf_name))


def physical_cores():
    """Distinct (physical id, core id) pairs of /proc/cpuinfo; None when the file does not say."""
    try:
        cores, phys, core = set(), None, None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                phys = line.split(":")[1].strip()
            elif line.startswith("core id"):
                core = line.split(":")[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    cores.add((phys, core))
                phys = core = None
        if phys is not None and core is not None:
            cores.add((phys, core))
        return len(cores) or None
    except OSError:
        return None


def cpu_baseline(r, args, maps):
    """The CPU oracle (a port of the reference algorithm, NOT Taichi's ti.cpu) on a bounded sample of the same workload:
    the full frame at --cpu-spp samples per pixel, same maps / camera / seed, all host threads."""
    import ctypes
    from digital_earth_amd import luts
    from oracle import oracle_binding as ob
    W, H = r.image_res
    o = ob.Oracle(W, H)
    names, crf = luts.load_crfs()
    o.upload_luts(luts.load_cie(), luts.load_srgb2spec(), luts.load_o3(), crf)
    for s in range(7):
        o.upload_texture(s, maps[s])
    p = ob.DeParams()
    ctypes.memmove(ctypes.byref(p), ctypes.byref(r._params), ctypes.sizeof(p))
    o.set_params(p)
    # bounded sample: 1 spp first; then as many more samples per pixel as fit in ~15 s (at most --cpu-spp, default 8)
    t0 = time.perf_counter()
    o.accumulate(1, r.seed)
    t1 = time.perf_counter() - t0
    extra = int(min(max(args.cpu_spp - 1, 0), max(0.0, 15.0 / max(t1, 1e-3) - 1.0)))
    if extra > 0:
        o.accumulate(extra, r.seed)
    dt = time.perf_counter() - t0
    args.cpu_spp = 1 + extra
    n = W * H * args.cpu_spp
    cores = physical_cores()
    out = {"value": n / dt / 1e6, "unit": "Msamples/s", "cores": cores if cores else o.threads, "threads": o.threads, "kind": "port",
           "cores_note": "physical cores of the host (/proc/cpuinfo); `threads` = OpenMP threads actually used (all hardware threads)" if cores
                         else "physical core count unavailable: `cores` = OpenMP threads used",
           "sample": "full %dx%d frame at %d spp (%d samples, %.1f s), same maps/camera/seed; C++ restatement of the "
                     "reference algorithm (oracle/), OpenMP over 16x8 pixel blocks" % (W, H, args.cpu_spp, n, dt)}
    # the same sample doubles as a full-size parity check of the GPU image (1 spp at matched seed)
    return out, o


def sparse_oracle_check(name, rk, maps, seed):
    """The frame `rk` holds (the config's FULL sample count) against the oracle on every `world`-th 8x8 tile: bit-identical fraction of those pixels."""
    import ctypes
    import numpy as np
    from digital_earth_amd import luts
    from oracle import oracle_binding as ob
    W, H = rk.image_res
    first, stride = SPARSE_CHECK[name]
    g = rk.fetch_hdr()
    o = ob.Oracle(W, H)
    _, crf = luts.load_crfs()
    o.upload_luts(luts.load_cie(), luts.load_srgb2spec(), luts.load_o3(), crf)
    for s in range(7):
        o.upload_texture(s, maps[s])
    p = ob.DeParams()
    ctypes.memmove(ctypes.byref(p), ctypes.byref(rk._params), ctypes.sizeof(p))
    o.set_params(p)
    t0 = time.perf_counter()
    o.accumulate_strided(rk.current_spp, seed, first, stride)
    dt = time.perf_counter() - t0
    mask = ob.Oracle.strided_mask(W, H, first, stride)
    c = o.fetch_hdr()
    same = float((c[mask].view(np.uint32) == g[mask].view(np.uint32)).mean())
    lit = float((c[mask] != 0).any(axis=-1).mean())
    del o
    return {"bit_identical_vs_oracle_on_sparse_tiles": same, "sparse_tiles": "every %dth 8x8 tile in raster order (from tile %d), %d pixels x %d spp, %.0f %% of them lit, oracle %.1f s" % (stride, first, int(mask.sum()), rk.current_spp, 100.0 * lit, dt)}


def write_outputs(path, frame):
    """--dump-outputs: the assembled HDR frame and its display image as the step left them (fetch_image re-runs the display transform, which is
    deterministic, on the same accumulation).  Above DUMP_LIMIT_BYTES a fixed seeded sample of pixels, the same for both arrays and every run."""
    import numpy as np
    arrays = {"hdr": frame.fetch_hdr(), "image": frame.r.fetch_image()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        n_pix = arrays["hdr"].shape[0] * arrays["hdr"].shape[1]
        idx = np.sort(np.random.default_rng(0).choice(n_pix, n_pix * DUMP_LIMIT_BYTES // total, replace=False))
        arrays = {k: a.reshape(n_pix, 3)[idx] for k, a in arrays.items()}
    os.makedirs(path, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(path, k + ".npy"), a.astype(np.float32, copy=False))


def run_other_config(name, r_main, maps, device_index, steps=2):
    """BASELINE cfg3 / cfg4 / cfg5 for a few steps on this GPU (after the timed cfg2 region, untimed by the contract): ms per step with frames back to back,
    the launch's own duration on a frame rendered alone, the §8(d) roofline fraction from THIS camera's tap counts, and the frame at the config's full
    sample count against the oracle on sparse tiles.  The maps are the resident ones (borrowed); cfg4 owns its cloud-heavy cloud map."""
    import numpy as np
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd import textures as T
    c = CONFIGS[name]
    W, H, spp = c["width"], c["height"], c["spp"]
    rk = Renderer((W, H), (0, 1, 0), device=device_index, texture_source="synthetic", texture_quality=2, cloud_heavy=c["cloud_heavy"], seed=0)
    try:
        apply_preset(rk, c["preset"], c["crf_name"])
        rk.share_textures_from(r_main)
        my_maps = maps
        if c["cloud_heavy"]:
            rk.copy_texture(T.CLOUDS)
            if maps is not None:
                my_maps = list(maps)
                my_maps[T.CLOUDS] = rk.download_texture(T.CLOUDS)
        rk.set_launch_slots(8, 3)
        rk.enable_counters(True)
        rk.reset_framebuffer()
        rk.accumulate(2)
        rk.synchronize()
        cnt = rk.counters()
        rk.enable_counters(False)
        n_r8, n_rgb = cnt["taps_r8"] / max(cnt["samples"], 1), cnt["taps_rgb8"] / max(cnt["samples"], 1)
        b_sample = 8.0 + 4.0 * n_r8 + 16.0 * n_rgb
        every = c["progressive"] if c["progressive"] > 0 else spp

        def step(lone=False):
            ms = 0.0
            rk.reset_framebuffer()
            done = 0
            while done < spp:
                n = min(every, spp - done)
                rk.accumulate(n)
                if lone:
                    rk.synchronize()
                    ms += rk.last_accumulate_ms()
                if c["progressive"] > 0:
                    rk.render_to_image_device()          # the progressive display after every K samples
                done += n
            if c["progressive"] <= 0:
                rk.render_to_image_device()
            return ms
        step()                                            # allocations of every launch slot: untimed
        rk.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        rk.synchronize()
        ms_per_step = (time.perf_counter() - t0) / steps * 1e3
        kernel_ms = step(lone=True)
        samples = W * H * spp
        out = {"workload": "%dx%d, %d spp%s, %s%s, quality-2 synthetic maps%s, BASELINE configs[%d]" % (W, H, spp, ", progressive display every %d" % every if c["progressive"] else "", c["preset"],
                                                                                                 " + film curve %s" % c["crf_name"] if c["crf_name"] else "", " (cloud-heavy)" if c["cloud_heavy"] else "", c["index"]),
               "metric": metric_name(W, H, spp, c["preset"], c["cloud_heavy"], c["progressive"]),
               "steps": steps, "ms_per_step": ms_per_step, "value": samples / (ms_per_step * 1e-3) / 1e6, "unit": "Msamples/s",
               "kernel_ms": kernel_ms, "launches_per_step": rk.last_call_info()["launches"] * ((spp + every - 1) // every),
               "bytes_per_sample": b_sample, "taps_r8_per_sample": n_r8,
               "roofline_frac": (b_sample * samples / (kernel_ms * 1e-3) / 1e9) / HBM_PEAK_GBPS}
        if my_maps is not None:
            out.update(sparse_oracle_check(name, rk, my_maps, rk.seed))
        return out
    finally:
        rk.close()


def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        # never silently run another configuration than the one asked for
        raise SystemExit("bench.py --gpus %d but WORLD_SIZE=%d: launch with `python -m torch.distributed.run --nnodes=1 "
                         "--nproc-per-node %d --master-addr 127.0.0.1 ... bench.py --gpus %d`" % (args.gpus, world, args.gpus, args.gpus))

    import numpy as np
    import torch
    import torch.distributed as dist
    from digital_earth_amd.renderer import Renderer
    from digital_earth_amd import parallel

    n_dev = max(torch.cuda.device_count(), 1)
    backend = None
    if world > 1:
        # "nccl" is RCCL on ROCm.  DE_DIST_BACKEND=gloo exercises the N > 1 code path with several ranks on ONE GPU
        # (RCCL refuses two ranks on one device); there parallel.reduce_hdr stages the buffer through host memory.
        backend = os.environ.get("DE_DIST_BACKEND", "nccl")
        if backend == "nccl" and n_dev < world:
            raise SystemExit("bench.py --gpus %d needs %d visible GPUs for RCCL, found %d (DE_DIST_BACKEND=gloo runs the ranks on one GPU)" % (world, world, n_dev))
    device_index = local_rank % n_dev          # one rank per GPU; the modulo only matters for the one-GPU gloo dry run
    torch.cuda.set_device(device_index)
    ranks_seen = 1
    if world > 1:
        kw = {"device_id": torch.device("cuda", device_index)} if backend == "nccl" else {}
        dist.init_process_group(backend=backend, rank=rank, world_size=world, **kw)
        if dist.get_world_size() != args.gpus:
            raise SystemExit("process group has %d ranks, --gpus %d" % (dist.get_world_size(), args.gpus))
        # count the ranks (and distinct devices) through the collective itself
        dev_t = torch.device("cuda", device_index) if backend == "nccl" else torch.device("cpu")
        seen = torch.zeros(world, dtype=torch.int64, device=dev_t)
        seen[rank] = 1 + device_index
        dist.all_reduce(seen)
        ranks_seen = int((seen > 0).sum().item())
        if ranks_seen != world:
            raise SystemExit("collective saw %d of %d ranks" % (ranks_seen, world))
        devices_seen = len(set(int(x) for x in seen.tolist()))
    else:
        devices_seen = 1

    W, H, spp = args.width, args.height, args.spp
    # Frames in flight: each has its own context (HDR / image buffers, work queue) and HIP stream; consecutive steps
    # alternate between them, so the tail of one frame (a few very long paths finishing) overlaps the start of the next.
    # Every step is still a complete frame (reset, spp samples per pixel, reduce, display).  The maps and LUTs are resident
    # ONCE per GPU: the second context borrows them (de_share_textures).
    frames = []
    tex_kw = dict(texture_source="synthetic", texture_quality=args.tex_quality, cloud_heavy=args.cloud_heavy, seed=0)
    if args.tex_size:
        tex_kw["texture_size"] = tuple(args.tex_size)
    for k in range(max(1, args.frames_in_flight)):
        rk = Renderer((W, H), (0, 1, 0), device=device_index, **tex_kw)
        if args.preset:
            apply_preset(rk, args.preset, args.crf_name)
        rk.set_integrator(args.integrator)
        if k == 0:
            rk.copy_textures()
        else:
            rk.share_textures_from(frames[0].r)
        if world > 1 and args.reduce == "lib":
            def exchange(uid):
                box = [uid]
                dist.broadcast_object_list(box, src=0)
                return box[0]
            frames.append(parallel.LibraryComm(rk, rank, world, exchange, split=args.split))
        else:
            frames.append(parallel.DistributedFrame(rk, rank, world, device_index, stream=torch.cuda.Stream(device=device_index, priority=-1), split=args.split, collective=args.collective))
        if args.simulate_world > 1 and world == 1:
            if args.split == "samples":
                rk.set_sample_partition(0, args.simulate_world)
            else:
                rk.set_tile_partition(0, args.simulate_world)
    r, frame = frames[0].r, frames[0]
    if args.standin_collective >= 0 and world == 1:
        for f in frames:
            f.standin_extra = args.standin_collective
    if args.cu_withhold > 0:
        for f in frames:
            t = f.r.tuning(); t.v6_cu_withhold = args.cu_withhold; f.r.set_tuning(t)
    # Launch settings.  Frames overlap through the library's launch slots (3 for frame-sized launches).  With N > 1 the collective
    # of frame k is then enqueued while frame k+1 renders: the render kernel's persistent waves own every vector register of the
    # CUs (5 per SIMD x 96 VGPRs), so the collective's kernel gets CUs as those waves drain (the frame's tail) — its stream has
    # the highest priority, so that freed wave slots go to it before the next frame's workgroups.  (Capping the waves per launch
    # does not leave room for it: 16 per CU cost 2 % on one GPU but the next launch in flight takes the free slots.)  Throughput
    # holds either way — the render launches do not wait for the collective — but the latency of a frame grows; `alt` below
    # times the same steps with one launch at a time, where the collective never queues behind a render.
    def apply_settings(serial, wpc):
        for f in frames:
            f.r.synchronize()
            f.r.set_launch_slots(1 if serial else 8, 1 if serial else 3)
            f.r.set_wave_budget(wpc)
    serial = bool(args.serial_frames)
    wpc = args.waves_per_cu if args.waves_per_cu > 0 else 20
    apply_settings(serial, wpc)
    # the CPU-baseline leg (after the timed region) needs the maps as uploaded: take them to the host now, then release the
    # 2.1 GB of as-uploaded device copies — the kernels read the packed copies only
    maps = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        maps = [r.download_texture(s) for s in range(7)]
    r.trim_textures()

    def barrier():
        for f in frames:
            f.r.synchronize()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    if args.full:
        # algorithmic work per sample, measured by the kernel's own counters on this camera/seed (untimed)
        r.enable_counters(True)
        r.reset_framebuffer()
        r.accumulate(2)
        r.synchronize()
        cnt = r.counters()
        r.enable_counters(False)
        n_r8 = cnt["taps_r8"] / max(cnt["samples"], 1)
        n_rgb = cnt["taps_rgb8"] / max(cnt["samples"], 1)

    # every context in flight allocates its per-sample buffer at its first full-size launch: prime them all (untimed), whatever
    # --warmup says, so that no allocation can fall into the timed region
    def step(f):
        if args.progressive > 0:
            f.render_frame_progressive(spp, args.progressive)
        else:
            f.render_frame(spp)

    def timed(n_steps):
        barrier()
        ta = time.perf_counter()
        for i in range(n_steps):
            step(frames[i % len(frames)])
            if args.sync_frames:
                frames[i % len(frames)].r.synchronize()
        barrier()
        return time.perf_counter() - ta

    # every launch slot of every context allocates its record buffer (and its pipe's queues) at its first launch: one frame per
    # launch slot and pipe (four pipes for a rank's share of the frame), untimed.  Nothing is measured or decided in these frames —
    # the launch policy no longer times kernels against each other (round 4) — so the count is a constant, reported in the line.
    n_prime = 4
    for f in frames:
        for _ in range(n_prime):
            step(f)
            if args.sync_frames:                 # (profiling runs: one call at a time from the first launch on, so that a kernel trace holds no launch that waited behind another call's persistent workgroups)
                f.r.synchronize()
    barrier()
    for i in range(args.warmup):
        step(frames[i % len(frames)])
        if args.sync_frames:
            frames[i % len(frames)].r.synchronize()
    elapsed = timed(args.steps)
    timed_info = frames[(args.steps - 1) % len(frames)].r.last_call_info()      # what the calls of the timed region ran (a lone call may run differently)
    last = frames[(args.steps - 1) % len(frames)]
    if args.dump_hdr and rank == 0:
        np.save(args.dump_hdr, last.r.fetch_hdr())
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, last)
    if world > 1:
        # the line's rate is the slowest rank's
        dev_t = torch.device("cuda", device_index) if backend == "nccl" else torch.device("cpu")
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev_t)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    total_samples = W * H * spp * args.steps
    value = total_samples / elapsed / 1e6
    ms_per_step = elapsed / args.steps * 1e3
    out = {
        "metric": "Msamples/sec (1920x1080, 64 spp) spectral path tracing" if args.config_name == "cfg2" else metric_name(W, H, spp, args.preset, args.cloud_heavy, args.progressive), "value": value, "unit": "Msamples/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "ranks_seen": ranks_seen, "devices_seen": devices_seen,
        "config": {"workload": "%dx%d, %d spp, full spectral Rayleigh+Mie+O3+clouds, quality-%d synthetic maps%s, %s, "
                               "%s" % (W, H, spp, args.tex_quality, " (%dx%d)" % tuple(args.tex_size) if args.tex_size else "",
                                                         (args.preset or "default camera") + (" + film curve %s" % args.crf_name if args.crf_name else "") + (", cloud-heavy maps" if args.cloud_heavy else ""),
                                                         "ray_marcher integrator (not the BASELINE metric)" if args.integrator != "path_tracer" else
                                                         ("BASELINE configs[%d]" % CONFIGS[args.config_name]["index"] if args.config_name else "not a BASELINE config")),
                   "parallelism": ((("tile-partition x%d + %s reduce (%s)" if args.collective == "reduce" else "tile-partition x%d + %s gather of the owned pixels (%s)") if args.split == "tiles" else "sample-partition x%d + %s rank-ordered gather-sum (%s)") % (world, "RCCL" if backend == "nccl" else backend, args.reduce)) if world > 1
                                  else ("single GPU" if args.simulate_world <= 1 else "single GPU rendering rank 0's share of a %s partition x%d (no collective)" % (args.split, args.simulate_world)),
                   "frames_in_flight": len(frames), "launch_slots": 1 if serial else 3,
                   "waves_per_cu": 24 if timed_info["variant"] == 6 else wpc,      # render_kernel_v6: two workgroups of 12 waves per CU (80 VGPRs); the wave budget knob belongs to the state machine
                   "primed_frames": n_prime,
                   "kernel": timed_info["kernel"], "launches_per_call": timed_info["launches"],
                   "progressive_every": args.progressive if args.progressive > 0 else None,
                   "samples_per_step": W * H * spp},
    }
    if args.cu_withhold > 0:
        out["config"]["cu_withhold_per_xcd"] = args.cu_withhold
    if not args.full:
        if rank == 0:
            print(json.dumps(out), flush=True)
        if world > 1:
            dist.barrier()
            for f in frames:
                f.close()
            dist.destroy_process_group()
        return

    # untimed: one frame at a time (latency of a single frame), with the HIP-event duration of its render launch
    per_launch, per_frame, per_reduce, per_drain = [], [], [], []
    for _ in range(max(1, min(args.steps, 3))):
        barrier()
        tf = time.perf_counter()
        frame.render_frame(spp)
        barrier()
        per_frame.append(time.perf_counter() - tf)
        per_launch.append(r.last_accumulate_ms())
        per_reduce.append(frame.last_reduce_ms() if world > 1 else 0.0)
        try:
            per_drain.append(r.last_launch_phases())      # render_kernel_v6's own clock: (launch, drain) of this frame's launch
        except Exception:
            pass
    avg_kernel_ms = float(np.mean(per_launch))
    single_frame_ms = float(np.mean(per_frame)) * 1e3
    my_render_ms, my_reduce_ms = avg_kernel_ms, float(np.mean(per_reduce))
    my_drain_ms = float(np.mean([d[1] for d in per_drain])) if per_drain else None

    # N > 1: the same K steps under the OTHER launch setting (serial <-> overlapping), untimed by the contract, reported as `alt`
    alt = None
    if world > 1:
        alt_serial = not serial
        alt_wpc = wpc
        apply_settings(alt_serial, alt_wpc)
        for _ in range(2):
            step(frame)
        alt_elapsed = timed(args.steps)
        alt = {"serial_frames": alt_serial, "waves_per_cu": alt_wpc, "elapsed_s": alt_elapsed}
        apply_settings(serial, wpc)

    multi = None
    if world > 1:
        dev_t = torch.device("cuda", device_index) if backend == "nccl" else torch.device("cpu")
        t = torch.tensor([elapsed, avg_kernel_ms, single_frame_ms, alt["elapsed_s"]], dtype=torch.float64, device=dev_t)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed, avg_kernel_ms, single_frame_ms, alt["elapsed_s"] = (float(x) for x in t.tolist())
        # what every rank measured on its own (HIP events): render launch, collective; and the tiles it owns
        per_rank = [None] * world
        info = timed_info
        dist.all_gather_object(per_rank, {"rank": rank, "render_ms": my_render_ms, "reduce_ms": my_reduce_ms,
                                          "drain_ms": my_drain_ms,      # of render_ms: from the first wave that found no work item left to the last wave's exit (a lone frame)
                                          "tiles_owned": int(parallel.tiles_per_rank(W, H, world)[rank]) if args.split == "tiles" else (W // 8) * (H // 8),
                                          "samples_per_pixel": spp if args.split == "tiles" else len(range(rank, spp, world)),
                                          "kernel": info["kernel"], "launches_per_call": info["launches"]})
        if args.check_spp > 0:
            # parity of the N-rank path on THIS hardware: the assembled frame must equal a 1-rank render bit for bit.
            # Untimed and after the measurement; a failure here is reported in the line, it does not lose the measurement.
            try:
                frame.render_frame(args.check_spp)
                barrier()
                if rank == 0:
                    assembled = frame.r.fetch_hdr()
                    solo = Renderer((W, H), (0, 1, 0), device=device_index, **tex_kw)     # a 1-rank render of the same frame
                    if args.preset:
                        apply_preset(solo, args.preset, args.crf_name)
                    solo.set_integrator(args.integrator)
                    solo.share_textures_from(r)
                    solo.accumulate(args.check_spp)
                    solo_hdr = solo.fetch_hdr()
                    solo.close()
                    multi = {"spp": args.check_spp,
                             "bit_identical_fraction": float((assembled.view(np.uint32) == solo_hdr.view(np.uint32)).mean()),
                             "rel_l2": float(np.sqrt(((assembled.astype(np.float64) - solo_hdr) ** 2).sum()) / max(np.sqrt((solo_hdr.astype(np.float64) ** 2).sum()), 1e-300)),
                             "nonzero_pixels": int((assembled != 0).any(axis=2).sum()),
                             "note": "tile partition: x + 0, bit-identical by construction; sample partition: rank-ordered partial sums, f32 re-association only (rel_l2 <= 1e-6)"}
                barrier()
            except Exception as exc:          # noqa: BLE001 - reported, not swallowed
                multi = {"spp": args.check_spp, "error": "%s: %s" % (type(exc).__name__, exc)}

    # roofline of the dominant kernel: algorithmic bytes per launch / measured launch duration.
    # B_sample = 8 B contribution record + 4 B per r8 tap + 16 B per colour tap (render_kernel_v2 writes one
    # 8-byte (radiance, wavelength node) record per sample, the HDR read-modify-write of 24 B per pixel per launch happens
    # in accumulate_kernel); samples per launch on this rank = its share of the frame.
    sim_world = args.simulate_world if (args.simulate_world > 1 and world == 1) else world
    sim_rank = 0 if (args.simulate_world > 1 and world == 1) else rank
    if args.split == "samples":
        my_samples = W * H * len(range(sim_rank, spp, sim_world))
    else:
        my_samples = int(parallel.owned_pixel_mask(W, H, sim_rank, sim_world).sum()) * spp
    b_sample = 8.0 + 4.0 * n_r8 + 16.0 * n_rgb
    achieved_gbps = b_sample * my_samples / (avg_kernel_ms * 1e-3) / 1e9
    traffic = None
    valu_insts = lane_util = salu_insts = None
    prof_name = None
    traffic_note = "not collected in this run (see profiles/ for the rocprofv3 --pmc pass)"
    prof = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    if os.path.exists(prof):
        try:
            with open(prof) as f:
                pj = json.load(f)
            if pj.get("workload") == "%dx%d_%dspp_q%d" % (W, H, spp, args.tex_quality) and world == 1 and not args.preset and not args.cloud_heavy and args.progressive <= 0 \
                    and not args.tex_size and args.simulate_world <= 1 and args.integrator == "path_tracer":
                # the counters belong to the kernel build that was profiled: refuse them when this run's launch duration is
                # not the profile's (+-8 %) — a changed kernel with an unrefreshed profile must not carry stale numbers
                prof_ms = pj.get("kernel_ms")
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                from summarize_profile import source_sha16
                same_sources = pj.get("source_sha16") == source_sha16()
                # admitted when the library's sources are the profiled ones (sha256 over csrc/) and the launch duration is within 8 %: boxes of the
                # pool differ by up to 5 % for one build (round 5), so the duration alone cannot tell a changed kernel from a slower box
                if prof_ms and same_sources and abs(avg_kernel_ms - prof_ms) <= 0.08 * prof_ms:
                    traffic = pj.get("hbm_bytes_per_launch")
                    traffic_note = ("REPLAYED, not measured in this run: `traffic` and the `valu.issue` block come from the committed rocprofv3 --pmc "
                                    "passes of this workload (profiles/hbm_traffic.json, profile %s), admitted because the library's sources are the profiled "
                                    "ones (sha256 over csrc/) and this run's launch duration is within 8 %% of the profiled one.  " % pj.get("profile")) + pj.get("note", "")
                    valu_insts, lane_util = pj.get("valu_insts_per_launch"), pj.get("valu_lane_utilisation")
                    salu_insts = pj.get("salu_insts_per_launch")
                    prof_name = pj.get("profile")
                else:
                    traffic_note = ("profiles/hbm_traffic.json (profile %s) is for a launch of %s ms of sources %s; this run measured %.1f ms on sources %s: counters "
                                    "withheld as stale" % (pj.get("profile"), prof_ms, pj.get("source_sha16"), avg_kernel_ms, source_sha16()))
        except Exception:
            pass

    steps_per_sample = (cnt["sphere_steps"] + cnt["tracking_steps"]) / max(cnt["samples"], 1)
    out.update({
        "single_frame_ms": single_frame_ms, "single_frame_value": W * H * spp / (single_frame_ms * 1e-3) / 1e6,
        "drain_ms": my_drain_ms,
        # `bound` names the roof that BINDS this kernel (VALU issue: `valu.issue` below); achieved / peak / unit / frac keep SURVEY §8(d)'s definition —
        # algorithmic bytes over the launch's duration against the HBM peak — and `hbm_frac` repeats that fraction under its own name
        "roofline": {"bound": "valu_issue", "achieved": achieved_gbps, "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": achieved_gbps / HBM_PEAK_GBPS, "hbm_frac": achieved_gbps / HBM_PEAK_GBPS,
                     # `achieved` divides by the launch's own duration (HIP events around one frame rendered alone): the non-overlapped figure.
                     # With frames back to back the next launch fills CUs as this one drains; the same bytes over ms_per_step:
                     "frac_single_frame": achieved_gbps / HBM_PEAK_GBPS,
                     "frac_overlapped_frames": (b_sample * my_samples / (ms_per_step * 1e-3) / 1e9) / HBM_PEAK_GBPS,
                     "traffic": traffic, "traffic_note": traffic_note,
                     "kernel": ("de_accumulate(%d): kernel variant %s — %s; "
                                "kernel_ms = the call's duration (HIP events on its launch slot: v6_kernel<.., false> — the frame's launch — + v6_kernel<.., true>, its 64-workgroup tail launch, back to back)" % (spp, os.environ.get("DE_KERNEL", "4 (automatic)"), timed_info["kernel"])) if args.integrator == "path_tracer" else "ray_march_kernel<false, 0>", "kernel_ms": avg_kernel_ms, "bytes_per_sample": b_sample,
                     "taps_r8_per_sample": n_r8, "taps_rgb_per_sample": n_rgb,
                     "note": "the path is VALU-issue / divergence bound, not HBM bound (SURVEY §8d): see valu"},
        "valu": {"unit": "see fields", "loop_steps_per_sample": steps_per_sample,
                 "sphere_steps_per_sample": cnt["sphere_steps"] / max(cnt["samples"], 1),
                 "tracking_steps_per_sample": cnt["tracking_steps"] / max(cnt["samples"], 1),
                 "vertices_per_sample": cnt["vertices"] / max(cnt["samples"], 1)},
    })
    if args.standin_collective >= 0 and world == 1:
        out["standin_collective"] = {"extra_copies": args.standin_collective, "queue_to_finish_ms_mean_of_last_16": r.last_reduce_ms(),
                                     "bytes": (3 + 2 * args.standin_collective) * W * H * 12,
                                     "note": "one-GPU stand-in for an N-rank run's per-frame collective, enqueued on the context stream where the reduce goes (include/digital_earth_debug.h)"}
    if multi is not None:
        out["multi_gpu_parity"] = multi
    if world > 1:
        out["per_rank"] = per_rank
        alt["value"] = total_samples / alt["elapsed_s"] / 1e6
        alt["ms_per_step"] = alt["elapsed_s"] / args.steps * 1e3
        out["alt"] = alt
    if valu_insts:
        # The bound that holds is VALU issue.  Instructions per launch = SQ_INSTS_VALU of the committed rocprofv3 --pmc pass
        # of this workload (profiles/); active lanes per instruction = its SQ_THREAD_CYCLES_VALU / (64 SQ_ACTIVE_INST_VALU).
        # Two ceilings are quoted: the guide's 2 cycles per wave64 f32 instruction per SIMD-32 at 2.4 GHz, and the rate
        # measured on this chip with independent instruction streams at the kernel's occupancy (tools/micro/dep_latency.hip: one
        # instruction per 1.00 ns per SIMD at the 6 waves per SIMD render_kernel_v6 runs — 1.05 ns at 5, 1.11 ns at 4).
        ach_ginst = valu_insts / (avg_kernel_ms * 1e-3) / 1e9
        peak_meas = 256 * 4 / 1.00
        peak_guide = 256 * 4 * 2.4 / 2.0
        lane_ops_per_sample = valu_insts * 64.0 * lane_util / my_samples
        out["valu"]["issue"] = {"achieved": ach_ginst, "unit": "1e9 wave64 VALU instructions/s",
                                "peak_measured": peak_meas, "frac_of_measured": ach_ginst / peak_meas,
                                "peak_guide": peak_guide, "frac_of_guide": ach_ginst / peak_guide,
                                "insts_per_launch": valu_insts, "lane_utilisation": lane_util, "profile": prof_name}
        if salu_insts:
            # what a scalar instruction costs beside the vector ones depends on the operating point: round 5's same-box builds (5.7 x the fabric traffic) put it
            # at ~0.6 of a vector instruction; round 6's (profiles/experiments: the busy flag as a VGPR, -16 % scalar / +1.4 % vector instructions, slower) at
            # less than a third.  Both weights are quoted; the vector rate alone (frac_of_measured) is the firm number.
            out["valu"]["issue"]["scalar_insts_per_launch"] = salu_insts
            out["valu"]["issue"]["frac_of_measured_with_scalar_at_0.6"] = (valu_insts + 0.6 * salu_insts) / (avg_kernel_ms * 1e-3) / 1e9 / peak_meas
            out["valu"]["issue"]["frac_of_measured_with_scalar_at_0.3"] = (valu_insts + 0.3 * salu_insts) / (avg_kernel_ms * 1e-3) / 1e9 / peak_meas
        out["valu"]["lane_ops_per_sample"] = lane_ops_per_sample
        out["valu"]["achieved_tlaneops"] = lane_ops_per_sample * my_samples / (avg_kernel_ms * 1e-3) / 1e12
        out["valu"]["peak_tlaneops"] = 256 * 4 * 32 * 2.4e9 / 1e12
        out["valu"]["frac"] = out["valu"]["achieved_tlaneops"] / out["valu"]["peak_tlaneops"]

    if (rank == 0 and world == 1 and args.config_name == "cfg2" and not args.no_other_configs and not args.tex_size and args.integrator == "path_tracer"
            and args.simulate_world <= 1 and len(frames) == 1 and not serial):
        # The other three BASELINE configs on this box, after the timed region and outside it: a few steps each (VERDICT r5 #4 — cfg3 / cfg4 / cfg5 had
        # builder-run numbers only).  A failure of a leg is reported in its entry; it never costs the cfg2 measurement.
        others = {}
        for name in ("cfg3", "cfg4", "cfg5"):
            try:
                others[name] = run_other_config(name, r, maps, device_index)
            except Exception as exc:          # noqa: BLE001 - reported, not swallowed
                others[name] = {"error": "%s: %s" % (type(exc).__name__, exc)}
        out["other_configs"] = others
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        base, o = cpu_baseline(r, args, maps)
        out["cpu_baseline"] = base
        # full-size parity at matched seed: GPU frame vs the CPU frame just computed
        r.set_tile_partition(0, 1)
        r.reset_framebuffer()
        r.accumulate(args.cpu_spp)
        g = r.fetch_hdr().astype(np.float64)
        c = o.fetch_hdr().astype(np.float64)
        # the product's second kernel (the state machine: calls below 4096 paths, counting launches) faces the CPU frame as well
        r.set_kernel_variant(2)
        r.reset_framebuffer()
        r.accumulate(args.cpu_spp)
        g3 = r.fetch_hdr().astype(np.float64)
        r.set_kernel_variant(int(os.environ.get("DE_KERNEL", "4")))
        out["parity"] = {"rel_l2_vs_cpu_port": float(np.sqrt(((g - c) ** 2).sum()) / max(np.sqrt((c ** 2).sum()), 1e-300)),
                         "bit_identical_fraction": float((g == c).mean()), "spp": args.cpu_spp,
                         "bit_identical_fraction_state_machine": float((g3 == c).mean()),
                         "note": "vs oracle/ (the build's CPU restatement): 0.0, every pixel bit-identical.  The oracle is held to the reference's own text EXECUTED under a Taichi stand-in "
                                 "(tests/golden/ref_*.npz, numpy f32 transcendentals, literal divisions): samples whose control flow agrees match to a median 2e-7, frames over them to "
                                 "2e-6 .. 1e-5 relative L2 (north star: 1e-3); 0 .. 5e-4 of the samples take another branch (an ulp of exp / log / atan2 flips a `rand < p` test) and are "
                                 "different paths — WHOLE-frame relative L2 of the 64x32 x 2 spp fixture frames, those samples included: 1.4e-3 / 3.8e-6 / 1.2e-5 / 3.9e-6 (default / florida / "
                                 "sunset / Apollo cameras; tests assert <= 1e-2).  By the fast-math scaling law (profiles/r5_fast_math.md: L2 ~ 1.5 sqrt(f / spp) for a fraction f of flipped "
                                 "samples) a 64-spp frame at f = 2e-4 .. 5e-4 sits at 3e-3 .. 4e-3 if the flipped samples carry typical radiance: '1e-3 at matched seed' holds sample by sample "
                                 "where the control flow agrees and cannot hold for whole frames against ANY implementation whose transcendentals differ in the last ulp from the one that drew "
                                 "the reference image.  Taichi-internal arithmetic (RNG, sampler, driver transcendentals) is defined, not pinned: DESIGN §2"}
        out["speedup_vs_cpu_port"] = value / base["value"]
    if world > 1 and (backend == "nccl" or os.environ.get("DE_FORCE_LIB_LEG")) and args.reduce == "torch" and args.check_spp > 0 and not os.environ.get("DE_NO_LIB_LEG"):
        # The library's own communicator (de_comm_init / de_reduce: RCCL bound with dlopen, ncclCommInitRank declared by hand) has
        # never run between two GPUs on the builder's box: give it ONE untimed frame here, after everything that is measured, and
        # report whether its assembled frame equals the torch.distributed one bit for bit.  A watchdog prints the line without it
        # if the leg hangs: the measurement is never hostage to this check.
        import threading

        printed = []
        print_lock = threading.Lock()

        def emit():
            # the line goes out exactly once, whichever of the main thread and the watchdog gets here first
            with print_lock:
                if rank == 0 and not printed:
                    print(json.dumps(out), flush=True)
                    printed.append(True)

        def bail():
            # this rank (or a peer it waits for) hangs in the leg, or in the barrier after it: the measurement is kept — the line goes out with
            # the failure in it — and the process ends NON-ZERO on every rank, so that a launcher sees the hang as a failure.
            # No restart / re-exec: the process has touched the GPU.
            out.setdefault("lib_reduce", {"error": "timed out after 120 s (rank %d)" % rank})
            emit()
            sys.stderr.write("bench.py: rank %d: the in-library RCCL leg (or the barrier after it) did not return within 120 s\n" % rank)
            sys.stderr.flush()
            os._exit(3)
        dog = threading.Timer(120.0, bail)
        dog.daemon = True
        dog.start()
        try:
            frame.render_frame(args.check_spp)
            barrier()
            ref_hdr = frame.r.fetch_hdr() if rank == 0 else None
            lr = Renderer((W, H), (0, 1, 0), device=device_index, **tex_kw)
            if args.preset:
                apply_preset(lr, args.preset, args.crf_name)
            lr.set_integrator(args.integrator)
            lr.share_textures_from(r)

            def exchange(uid):
                box = [uid]
                dist.broadcast_object_list(box, src=0)
                return box[0]
            lf = parallel.LibraryComm(lr, rank, world, exchange)
            lf.render_frame(args.check_spp)
            lr.synchronize()
            if rank == 0:
                lib_hdr = lf.fetch_hdr()
                out["lib_reduce"] = {"spp": args.check_spp, "reduce_ms": lf.last_reduce_ms(),
                                     "bit_identical_fraction": float((lib_hdr.view(np.uint32) == ref_hdr.view(np.uint32)).mean())}
            dist.barrier()
            lf.close()
        except Exception as exc:          # noqa: BLE001 - reported, not swallowed
            out["lib_reduce"] = {"error": "%s: %s" % (type(exc).__name__, exc)}
        emit()
        dist.barrier()                    # still under the watchdog: a peer that died in the leg must not hang this rank
        for f in frames:
            f.close()
        dist.destroy_process_group()
        dog.cancel()
        return
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        for f in frames:
            f.close()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
