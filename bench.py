#!/usr/bin/env python3
"""Benchmark: Msamples/s of the MI355X wavefront `path` integrator.

Workload (BASELINE.json metric "Msamples/sec at 1280x720x256spp"): config C3,
the synthetic ~1M-triangle instanced-bunny scene (scenes/bunny15.xml:
1,041,765 triangles, roughconductor Cu GGX 0.2, maxDepth 8, rrDepth 5,
gaussian hdrfilm) at 1280x720x256 spp.  One step = one full frame
(235,929,600 samples) rendered into an HBM-resident ImageBlock and copied to
the host.  Scene load, kd-tree build and upload are excluded (as Mitsuba
logs them separately, renderjob.cpp:102,113).

Multi-GPU (config C4): one process per GPU; the film's 16x16 tiles are dealt
round-robin (deal key k -> rank k % N); no collective touches the data path.
After the timed region every rank's per-tile ImageBlocks are gathered to rank 0
over gloo and put into the frame (ImageBlock::put, imageblock.h:103-107); the
parity leg runs on that assembled frame, and rank 0 checks it against a
whole-frame render of its own GPU.  Total work is the fixed frame, so scaling
is "strong".  `--gpus N` without a launcher starts the N ranks itself (through
torch.distributed.run, before any GPU call) and refuses to run when fewer than
N GPUs are visible, unless --allow-shared is given (a rehearsal of N ranks on
fewer GPUs; the line then says so).

A plain run sets up, warms up, times the steps and prints the result line
(value, ms_per_step and the timed steps' per-kernel HIP-event times).  --full
adds the legs that take runs of their own after the timed region: the
instrumented pass behind the roofline figures and the committed PMC sets they
quote, the parity leg against the CPU oracle, the CPU baseline and, for N > 1
ranks, the check of the assembled frame against a whole-frame render
(--no-count, --no-parity and --no-cpu drop single legs of a --full run).
--dump-outputs DIR writes the ImageBlock of the timed steps' last frame
(rank 0: the frame assembled from every rank's tiles) as DIR/imageblock.npy,
float32 [H + 2b, W + 2b, 5]; the scene, the frame and the counter-mode random
numbers are the same from run to run.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--workload bunny15|cbox|c5] [--full] [--dump-outputs DIR]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "my-mitsuba_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec (MI355X_MICROARCH.md)


def trace_kernel(a):
    """rocprofv3's name of the timed traversal instantiation this run launches
    (the instrumented COUNT pass runs k_trace_s<true, ...>)."""
    return "k_trace_s<false, 16, true, false>" if a.instancing == "two-level" else "k_trace_s<false, 16, false, false>"


def device_build_id():
    """The device library this run loads (MTSG_LIB or the in-tree
    libmtsg.so): the first 16 hex digits of its SHA-256."""
    import hashlib
    alt = os.environ.get("MTSG_LIB")
    path = os.path.join(REPO, alt) if alt else os.path.join(REPO, "my-mitsuba_amd", "libmtsg.so")
    try:
        return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]
    except OSError:
        return None


def pmc_key(a, world=1):
    """The configuration a committed PMC set must have been collected on for
    this run to quote it (tools/gpu_pmc_config.sh, tools/pmc_kernels.py):
    the workload, its size and share, the batch and tail-kernel settings and
    the device library's build -- counters of another build or batch size
    describe other launches and are never quoted."""
    key = {"workload": a.workload, "instancing": a.instancing, "kd_build": a.kd_build, "width": a.width,
           "height": a.height, "spp": a.spp, "share": max(world, a.emulate_ranks, 1),
           "batch_paths": a.batch_paths or 0, "finish_paths": a.finish_paths,
           "balance_rounds": a.balance_rounds if max(world, a.emulate_ranks, 1) > 1 else 0, "build": device_build_id()}
    if getattr(a, "kd_props", ""):
        key["kd_props"] = a.kd_props   # another tree: other launches
    if getattr(a, "finish_shade_min", 0) > 0:
        key["finish_shade_min"] = a.finish_shade_min
    if getattr(a, "lanes", 0) > 0 or getattr(a, "stagger", -1) >= 0:
        key["lanes"] = [getattr(a, "lanes", 0), getattr(a, "stagger", -1)]   # other launch sequence
    return key


def pmc_lookup(key, directory=None):
    """The newest committed per-kernel PMC set (profiles/rNN_pmc_*.json) whose
    key equals this run's configuration, or (None, None).  PMC counters need
    their own profiler runs (MI355X_MICROARCH.md), so they cannot be read
    live; a set of another configuration is never used."""
    import glob
    files = sorted(glob.glob(os.path.join(directory or os.path.join(REPO, "profiles"), "r*_pmc_*.json")))
    for f in reversed(files):
        try:
            j = json.load(open(f))
        except (OSError, ValueError):
            continue
        if j.get("key") == key:
            return j, os.path.relpath(f, REPO)
    return None, None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--allow-shared", action="store_true",
                    help="N>1: allow ranks to share GPUs when fewer than N are visible (rehearsal only)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="bunny15", choices=["bunny15", "cbox", "c5"])
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--kd-build", default="host", choices=["host", "device"],
                    help="top-level kd-tree: the host SAH build (default) or the GPU build (mtsg_kd_build)")
    ap.add_argument("--instancing", default="flatten", choices=["flatten", "two-level"],
                    help="C3's 15 bunny instances: world-space copies in one tree, or Mitsuba's two-level structure")
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--batch-paths", type=int, default=0)
    ap.add_argument("--finish-paths", type=int, default=-1,
                    help="tail-mode threshold (paths; 0 = off; default: the library's, mtsg_set_finish_paths)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the roofline's instrumented pass (and quote the committed "
                         "PMC sets), the parity leg, the CPU baseline and, for N > 1 ranks, the assembly check")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the ImageBlock of the timed steps' last frame to DIR/imageblock.npy (float32; rank 0)")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline leg")
    ap.add_argument("--no-parity", action="store_true", help="--full: skip the headline parity leg")
    ap.add_argument("--parity-stride", type=int, default=8,
                    help="parity leg: compare the 16x16 tiles t %% N == 0 (1/N of the frame) at full spp")
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="target CPU-baseline sample time")
    ap.add_argument("--emulate-ranks", type=int, default=0,
                    help="single process: render only rank 0's tile share of an N-GPU run (scaling rehearsal)")
    ap.add_argument("--balance-rounds", type=int, default=4,
                    help="shares > 1: warm-up rounds that re-cut the ranks' tile shares from their measured step "
                         "times (mtsg_set_tile_list); 0 = the fixed stride deal")
    ap.add_argument("--save", default="", help="write the developed image (.npy) here (rank 0)")
    ap.add_argument("--no-count", action="store_true",
                    help="--full: skip the instrumented (untimed) pass of per-ray counts (profiler runs)")
    ap.add_argument("--print-pmc-key", action="store_true", help="print this configuration's PMC key and exit")
    ap.add_argument("--pmc-pass", action="store_true",
                    help="profiler pass (tools/gpu_pmc_config.sh): render only this configuration's frame -- share 0 "
                         "of the stride deal when shares are emulated -- warmup + steps times, no balancing, no "
                         "whole-frame timing, no instrumented pass; prints the frame count")
    ap.add_argument("--share-layout", default="spread", choices=["spread", "bands"],
                    help="balanced shares cut runs of: the golden-ratio key order (spread over the frame) or the "
                         "row-major key order (each share a band of tile rows, its XCD ranges sub-bands)")
    ap.add_argument("--ray-order", type=int, default=-1, choices=[-1, 0, 1],
                    help="MTSG_OPT_RAY_ORDER: 1 = bounce rays in direction-sorted windows, 0 = append order (default)")
    ap.add_argument("--finish-shade-min", type=int, default=0,
                    help="tail kernel: a wave shades once this many of its busy lanes wait to (MTSG_OPT_FINISH_SHADE_MIN; 0 = the default, 16)")
    ap.add_argument("--lanes", type=int, default=0,
                    help="batches in flight on their own streams (MTSG_OPT_LANES; 0 = the library's default, 1)")
    ap.add_argument("--stagger", type=int, default=-1, help="bounces between the lanes' starts (MTSG_OPT_STAGGER)")
    ap.add_argument("--kd-props", default="",
                    help="scene kd-tree properties for the build, k=v[,k=v] (scene.cpp:47-83 names: "
                         "kdIntersectionCost, kdTraversalCost, kdEmptySpaceBonus, kdStopPrims, ...; measurement)")
    ap.add_argument("--shade-generic", action="store_true",
                    help="shade with the all-materials kernel instead of the scene's material set (A/B measurement)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return a


def visible_gpus():
    """GPUs visible to this process, counted without initialising the GPU
    (torch.cuda.device_count() does not on this image; HIP_VISIBLE_DEVICES and
    ROCR_VISIBLE_DEVICES apply)."""
    import torch
    return torch.cuda.device_count()


def launch_ranks(a, argv):
    """`bench.py --gpus N` run without a launcher: start the N ranks as children
    (torch.distributed.run, one process per GPU, rendezvous on 127.0.0.1) and
    return their exit code.  Nothing here touches the GPU, so the children are
    started from a process that never initialised it."""
    import socket
    import subprocess
    n = visible_gpus()
    if n < a.gpus and not a.allow_shared:
        raise SystemExit(f"bench.py --gpus {a.gpus}: only {n} GPU(s) visible; refusing to run {a.gpus} ranks "
                         f"on them (--allow-shared rehearses N ranks on fewer GPUs)")
    if n < 1:
        raise SystemExit("bench.py: no GPU visible")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__), *argv]
    return subprocess.call(cmd)


def dist_setup(n):
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", str(rank)))
    if world != n and world > 1:
        raise SystemExit(f"--gpus {n} but WORLD_SIZE={world}")
    pg = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # gloo: host-side barrier / max-reduce of the timings only; no data-path collective
        dist.init_process_group("gloo", rank=rank, world_size=world)
        pg = dist
    return rank, world, local, pg


def barrier(pg):
    if pg is not None:
        pg.barrier()


def max_over_ranks(pg, x):
    if pg is None:
        return x
    import torch
    t = torch.tensor([x], dtype=torch.float64)
    pg.all_reduce(t, op=pg.ReduceOp.MAX)
    return float(t.item())


def scene_args(a):
    if a.workload == "c5":
        # C5: dielectric + rough copper bunnies under an HDR environment, maxDepth 64
        # (scenes/env_glass.xml; 1920x1080x1024 unless overridden)
        path = os.path.join(REPO, "scenes", "env_glass.xml")
        return path, {"width": a.width, "height": a.height, "spp": a.spp, "maxDepth": 64}
    path = os.path.join(REPO, "scenes", "bunny15.xml" if a.workload == "bunny15" else "cbox.xml")
    defs = {"width": a.width, "height": a.height, "spp": a.spp, "maxDepth": 8}
    return path, defs


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cgroup_cpus():
    """CPU quota of this process's cgroup (cpu.max), or None when unlimited."""
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        return None if q == "max" else round(int(q) / int(p), 2)
    except (OSError, ValueError):
        return None


def mitsuba_tree_scene(scene):
    """The same scene with Mitsuba's own kd-tree parameters (gkdtree.h:734-744:
    stopPrims 6; this build's GPU-tuned default is 4), so the CPU baseline
    traverses the tree Mitsuba would build."""
    import mtsg
    # the Scene's own kdStopPrims property (scene.cpp:64-65), as a Mitsuba
    # scene file or plugin would set it
    return mtsg.Scene(scene.path, scene.defines, instancing=scene.instancing, scene_props={"kdStopPrims": 6})


def cpu_baseline(scene, params, border, target_s):
    """Oracle (faithful C++ restatement, Mitsuba SSE2 flags, SFMT sampler,
    32x32 spiral blocks, one worker per core) timed on a bounded sample of
    the same frame: all pixels at a reduced spp chosen to take ~target_s.
    SURVEY §8(d): all host cores, best of 3 (kdbench.cpp:213-242 style); the
    box's per-GPU share of 16 cores is timed once beside it."""
    from oracle import pyoracle as O
    try:
        visible = len(os.sched_getaffinity(0))
    except AttributeError:
        visible = os.cpu_count() or 1
    # all host cores this process may use: the visible CPUs, capped by the
    # cgroup's CPU quota (the GPU box shows 256 CPUs but grants 16 per GPU;
    # more threads than the quota only time-slice)
    quota = cgroup_cpus()
    cores = max(1, min(visible, int(quota + 0.999))) if quota else visible
    scene = mitsuba_tree_scene(scene)
    p = params.copy()
    p.spp = 1
    _, st = O.render(scene.desc, p, border, rng=O.RNG_SFMT, threads=cores, fast=True)
    rate1 = st.samples / max(st.seconds, 1e-9)
    spp = int(max(1, min(params.spp, round(target_s * rate1 / (params.tile_w * params.tile_h)))))
    p.spp = spp
    runs = []
    for _ in range(3):
        _, st = O.render(scene.desc, p, border, rng=O.RNG_SFMT, threads=cores, fast=True)
        runs.append(st.samples / st.seconds)
    best = max(runs)
    rvis = None
    if visible != cores:
        _, stv = O.render(scene.desc, p, border, rng=O.RNG_SFMT, threads=visible, fast=True)
        rvis = stv.samples / stv.seconds
    return {
        "value": round(best / 1e6, 4), "unit": "Msamples/s", "cores": cores, "kind": "port",
        "cpu_model": cpu_model(), "nproc": os.cpu_count(), "cgroup_cpus": cgroup_cpus(),
        "runs_msamples_s": [round(r / 1e6, 4) for r in runs],
        "value_all_visible_threads": round(rvis / 1e6, 4) if rvis else None,
        "sample": f"{params.tile_w}x{params.tile_h}x{spp}spp of the same scene/frame "
                  f"({st.samples} samples per run, best of 3 on {cores} threads = min(visible CPUs {visible}, "
                  f"cgroup quota {quota}); oracle/liboracle_fast.so, "
                  f"-O3 -msse2 -march=nocona -funsafe-math-optimizations, SFMT independent sampler, "
                  f"32x32 spiral blocks)",
    }


def _share(params, stride, offset):
    p = params.copy()
    if stride > 1:
        p.tile_stride, p.tile_offset = stride, offset
    return p


def parity_keys(world, stride):
    """Deal keys the parity leg compares: k mod (world * stride) < world, i.e.
    1/stride of the frame's tiles with the same number from every rank (for
    world 1: k % stride == 0)."""
    return world * stride, world


def all_gather_obj(pg, obj, world):
    if pg is None:
        return [obj]
    out = [None] * world
    pg.all_gather_object(out, obj)
    return out


def gather_frame(pg, rank, world, part, tile_w, tile_h, border):
    """Host-side tile gather (no collective on the data path: it runs after
    the timed region): every rank's share -- ("win", its per-tile ImageBlocks,
    mtsg_render_device_tiles) or ("block", a block of the whole rectangle) --
    goes to rank 0 over gloo and is put into the frame's ImageBlock
    (ImageBlock::put, imageblock.h:103-107; BlockedRenderProcess's merge,
    imageproc.cpp:28-78).  Returns the frame on rank 0, None elsewhere."""
    import mtsg
    parts = [part]
    if pg is not None:
        parts = [None] * world if rank == 0 else None
        pg.gather_object(part, parts, dst=0)
    if rank != 0:
        return None
    frame = np.zeros((tile_h + 2 * border, tile_w + 2 * border, 5), np.float32)
    for r, (kind, arr, *rest) in enumerate(parts):
        keys = rest[0] if rest else None   # a tile list's keys (balanced shares), else the stride deal
        if kind == "win":
            mtsg.put_tile_windows(frame, arr, tile_w, tile_h, border, world, r, keys=keys)
        else:
            frame += arr
    return frame


def interior_pixels(sel, border):
    """The pixels of the selected tiles whose reconstruction-filter footprint
    (radius `border`) lies in selected tiles only: in the frame they receive
    samples of the selected tiles alone, as in the oracle's block of those
    tiles (outside the frame nothing is splatted on either side)."""
    h, w = sel.shape
    pad = np.pad(sel, border, constant_values=True)
    ok = sel.copy()
    for dy in range(-border, border + 1):
        for dx in range(-border, border + 1):
            ok &= pad[border + dy:border + dy + h, border + dx:border + dx + w]
    return ok


def parity_at_headline(scene, frame, params, border, stride, world):
    """Per-pixel L1 of the GPU frame vs the CPU oracle at the full spp.  `frame`
    is the ImageBlock the timed steps produced, assembled from every rank's
    tiles; the oracle renders the tiles of parity_keys (1/stride of the frame,
    every pixel of them, all samples) in counter mode (identical random numbers
    per pixel / sample / dimension); both are developed (sum w L / sum w) and
    compared on those of their pixels that receive no sample of another tile
    (interior_pixels).  Runs after the timed region."""
    import mtsg
    from oracle import pyoracle as O
    mod, below = parity_keys(world, stride)
    p = params.copy()
    p.tile_stride = mod
    img_c, samples = None, 0
    t0 = time.time()
    for r in range(below):
        p.tile_offset = r
        blk, st = O.render(scene.desc, p, border, rng=O.RNG_COUNTER)
        img_c = blk if img_c is None else img_c + blk
        samples += st.samples
    t_cpu = time.time() - t0
    b = border
    rgb_g = mtsg.develop(frame[b:b + p.tile_h, b:b + p.tile_w])
    rgb_c = mtsg.develop(img_c[b:b + p.tile_h, b:b + p.tile_w])
    own = interior_pixels((mtsg.tile_deal_keys(p.tile_w, p.tile_h) % mod) < below, border)
    d = np.abs(rgb_g - rgb_c)[own]
    l1 = float(d.mean())
    mean = float(rgb_c[own].mean())
    # per-pixel L1 (mean over RGB of |GPU - CPU|) and its distribution
    px = d.mean(-1)
    dist = {"p50": float(np.percentile(px, 50)), "p90": float(np.percentile(px, 90)),
            "p99": float(np.percentile(px, 99)), "p999": float(np.percentile(px, 99.9)), "max": float(px.max()),
            "frac_over_1e-3": float((px > 1e-3).mean()), "frac_over_1e-3_of_mean": float((px > 1e-3 * mean).mean())}
    return {"l1": l1, "mean": round(mean, 6), "l1_rel_mean": l1 / max(mean, 1e-12),
            "max_abs": float(d.max()), "per_pixel": dist, "pixels": int(own.sum()), "spp": int(p.spp),
            "samples": int(samples),
            "tiles": (f"16x16 tiles with deal key % {mod} < {below} of {p.tile_w}x{p.tile_h}, the pixels whose "
                      f"{2 * border + 1}x{2 * border + 1} filter window lies in those tiles"
                      + (f" ({below // world} per rank's share), from the frame assembled from all {world} ranks"
                         if world > 1 else ", from the timed steps' last frame")),
            "bar": "l1 < 1e-3 (and l1_rel_mean < 1e-3)", "pass": bool(l1 < 1e-3 and l1 < 1e-3 * max(mean, 1e-12)),
            "rng": "counter mode on both sides", "oracle_seconds": round(t_cpu, 1)}


def main():
    a = parse()
    if a.print_pmc_key:
        print(json.dumps(pmc_key(a, int(os.environ.get("WORLD_SIZE", "1")))))
        return
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(a, sys.argv[1:]))
    rank, world, local, pg = dist_setup(a.gpus)
    import mtsg
    # one GPU per rank (LOCAL_RANK); ranks share GPUs only with --allow-shared
    # (a rehearsal of the multi-process path on a smaller box)
    ndev = mtsg.device_lib().mtsg_device_count()
    if ndev < 1:
        raise SystemExit("bench.py: no gfx950 device visible")
    dev = local % ndev if world > 1 else 0
    devices = None
    if world > 1:
        # every rank sees every rank's device identity, so all refuse together
        ids = all_gather_obj(pg, mtsg.device_pci_id(dev), world)
        devices = {"distinct": len(set(ids)), "pci": ids, "shared": len(set(ids)) < world}
        if len(set(ids)) < world and not a.allow_shared:
            raise SystemExit(f"bench.py: {world} ranks but only {len(set(ids))} distinct GPU(s) ({ids}); "
                             "refusing (--allow-shared rehearses N ranks on fewer GPUs)")

    path, defs = scene_args(a)
    t_load = time.time()
    kd_props = {}
    for kv in filter(None, a.kd_props.split(",")):
        k, v = kv.split("=", 1)
        kd_props[k.strip()] = float(v) if "Cost" in k or "Bonus" in k else int(v)
    scene = mtsg.Scene(path, defs, instancing=a.instancing, scene_props=kd_props or None)
    load_s = time.time() - t_load
    kd_info = {"kd_build": "host", "kd_build_ms": round(scene.info.kd_build_seconds * 1e3, 1), "kd_refs": scene.info.kd_indices,
               "kd_stop_prims": kd_props.get("kdStopPrims", 4)}   # the build's GPU-tuned default; Mitsuba: 6
    if kd_props:
        kd_info["kd_props"] = kd_props
    if a.kd_build == "device":
        mtsg.kd_build(scene, device=dev)   # warm-up
        tree = mtsg.kd_build(scene, device=dev)
        scene.set_kdtree(tree)
        kd_info = {"kd_build": "device", "kd_build_ms": round(tree["ms"], 1), "kd_refs": int(tree["indices"].size),
                   "host_kd_build_ms": round(scene.info.kd_build_seconds * 1e3, 1)}
    border = scene.border
    params = scene.params()
    params.tile_stride = world
    params.tile_offset = rank
    if a.emulate_ranks > 1 and world == 1:
        params.tile_stride = a.emulate_ranks
    gpu = mtsg.GPUScene(scene, dev)
    if a.batch_paths:
        gpu.set_batch_paths(a.batch_paths)
    elif devices and devices["shared"]:
        # ranks sharing a GPU size their batches from free-memory snapshots
        # that can coincide: cap each rank at its share of 2^29 paths (148 GB)
        # so that together they fit the 288 GB HBM
        sharing = devices["pci"].count(devices["pci"][rank])
        gpu.set_batch_paths(max(1 << 20, (1 << 29) // sharing))
    if a.finish_paths >= 0:
        gpu.set_finish_paths(a.finish_paths)
    if a.shade_generic:
        gpu.set_option(mtsg.MTSG_OPT_SHADE_GENERIC, 1)
    if a.ray_order >= 0:
        gpu.set_option(mtsg.MTSG_OPT_RAY_ORDER, a.ray_order)
    if a.finish_shade_min > 0:
        gpu.set_option(mtsg.MTSG_OPT_FINISH_SHADE_MIN, a.finish_shade_min)
    if a.lanes > 0:
        gpu.set_option(mtsg.MTSG_OPT_LANES, a.lanes)
    if a.stagger >= 0:
        gpu.set_option(mtsg.MTSG_OPT_STAGGER, a.stagger)
    W, H = params.tile_w + 2 * border, params.tile_h + 2 * border
    nbytes = W * H * 5 * 4
    film = gpu.alloc(nbytes)
    host_block = np.zeros((H, W, 5), np.float32)

    # a rank whose share is a fraction of the tiles returns its tiles' own
    # ImageBlocks (mtsg_render_device_tiles: 16 + 2b square windows, the
    # per-block ImageBlocks of BlockedRenderProcess) instead of a block of the
    # whole frame: 3.6 MB instead of 18.7 MB over PCIe per 1/8 C3 share.  The
    # host puts them into the frame's block after the timed region.
    # Shares.  With --balance-rounds > 0 (default) a share is an explicit
    # list of deal keys (mtsg_set_tile_list): a run of balance_order, whose
    # length the warm-up rounds re-cut from the shares' measured step times
    # (the reference's scheduler gives the next block to whichever worker is
    # free, src/libcore/sched.cpp:427-496); without it, the stride deal.
    emulated = a.emulate_ranks > 1 and world == 1
    n_shares = a.emulate_ranks if emulated else world
    n_tiles = ((params.tile_w + 15) // 16) * ((params.tile_h + 15) // 16)
    # balancing cuts runs of at least one tile per share: with fewer tiles
    # than shares the stride deal is used (a share may then be empty)
    balanced = n_shares > 1 and a.balance_rounds > 0 and n_tiles >= n_shares
    order = mtsg.balance_order(n_tiles) if a.share_layout == "spread" else np.arange(n_tiles, dtype=np.int32)
    counts = np.array([len(range(r, n_tiles, n_shares)) for r in range(n_shares)], dtype=np.int64)
    cur = {"keys": None}

    def share_keys(r):
        lo = int(counts[:r].sum())
        return np.sort(order[lo:lo + int(counts[r])])

    def use_share(r):
        if balanced:
            cur["keys"] = share_keys(r)
            gpu.set_tile_list(cur["keys"])
        else:
            params.tile_stride, params.tile_offset = (n_shares, r) if n_shares > 1 else (1, 0)

    def use_whole():
        cur["keys"] = None
        gpu.set_tile_list(None)
        params.tile_stride, params.tile_offset = 1, 0

    def windows_for(p):
        n, w = gpu.tile_windows(p)
        return (n, w) if (cur["keys"] is not None or p.tile_stride > 1) and n * w * w < W * H else None
    # window buffer: room for any share the balancing may cut
    win_max = n_tiles if n_shares > 1 else 0
    wbuf = gpu.alloc(win_max * (16 + 2 * border) ** 2 * 5 * 4) if win_max else None
    host_win = np.zeros((max(1, win_max), 16 + 2 * border, 16 + 2 * border, 5), np.float32)

    def step():
        nw = windows_for(params)
        if nw:
            wbytes = nw[0] * nw[1] * nw[1] * 5 * 4
            mtsg.device_lib().mtsg_device_memset(gpu._h, wbuf, wbytes)
            gpu.render_device_tiles(params, wbuf)
            mtsg.device_lib().mtsg_device_to_host(gpu._h, host_win.ctypes.data, wbuf, wbytes)
            return
        mtsg.device_lib().mtsg_device_memset(gpu._h, film, nbytes)
        gpu.render_device(params, film)
        mtsg.device_lib().mtsg_device_to_host(gpu._h, host_block.ctypes.data, film, nbytes)

    if a.pmc_pass:
        # rocprofv3 counts every launch of the process: render exactly the
        # frames a PMC set is normalised by (tools/pmc_kernels.py), and nothing else
        if n_shares > 1:
            params.tile_stride, params.tile_offset = n_shares, 0
        for _ in range(a.warmup + a.steps):
            step()
        gpu.free(film)
        if wbuf is not None:
            gpu.free(wbuf)
        gpu.close()
        if rank == 0:
            print(json.dumps({"pmc_pass_frames": a.warmup + a.steps, "share": "0 of %d (stride deal)" % n_shares
                              if n_shares > 1 else "whole frame"}))
        return
    # --emulate-ranks N: every rank's tile share in turn on this one GPU, each
    # timed like a rank of an N-GPU run (max over the shares = the frame time)
    shares = list(range(a.emulate_ranks)) if emulated else [rank]
    balance_log = []
    if balanced:
        # warm-up rounds that re-cut the shares: every share renders one step
        # (the first, untimed, allocates), then the tile counts follow the
        # measured rates (mtsg.balance_cuts); every rank computes the same cuts
        # from the all-gathered times
        for r in shares:
            use_share(r)
            step()
        for _ in range(a.balance_rounds):
            times = {}
            for r in shares:
                use_share(r)
                # the faster of two steps: a share that grew past the batch
                # buffers reallocates them in its first step
                best = None
                for _ in range(2):
                    barrier(pg)
                    t0 = time.perf_counter()
                    step()
                    dt = time.perf_counter() - t0
                    best = dt if best is None else min(best, dt)
                times[r] = best
            if not emulated:
                times = dict(enumerate(all_gather_obj(pg, times[rank], world)))
            t = [times[r] for r in range(n_shares)]
            balance_log.append({"tiles": counts.tolist(), "ms": [round(x * 1e3, 3) for x in t]})
            counts = mtsg.balance_cuts(counts, t)
    share_s = []
    acc = {}
    for off in shares:
        use_share(off)
        for _ in range(a.warmup):
            step()
        # per-kernel HIP events on the library's stream stay on through the
        # timed steps (two event records per launch); the per-frame figures
        # are summed (rank 0's share only when shares are emulated)
        gpu.set_flags(mtsg.MTSG_FLAG_TIMING)
        barrier(pg)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
            st = gpu.stats()
            if off == shares[0]:
                for f in ("ms_trace_closest", "ms_trace_shadow", "ms_shade", "ms_camera", "ms_splat", "ms_total", "ms_sort",
                          "rays_closest", "rays_shadow", "launches_trace_closest", "launches_trace_shadow",
                          "ms_finish", "paths_finish", "launches_finish"):
                    acc[f] = acc.get(f, 0) + getattr(st, f)
        barrier(pg)
        share_s.append(time.perf_counter() - t0)
        gpu.set_flags(0)
    use_share(shares[0])
    elapsed = max_over_ranks(pg, max(share_s))
    whole_s = None
    if len(shares) > 1:
        # the whole frame on this GPU, for the per-share speedups
        use_whole()
        for _ in range(a.warmup):
            step()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            step()
        whole_s = time.perf_counter() - t0
        use_share(shares[0])
    samples_total = params.tile_w * params.tile_h * params.spp * a.steps
    value = samples_total / elapsed / 1e6
    ms_per_step = elapsed / a.steps * 1e3

    # ---- roofline of the traversal kernel: HIP-event times of the timed
    # steps, algorithmic work from an instrumented (untimed) pass
    roofline = None
    kernels = {}
    if rank == 0:
        k = a.steps
        kernels = {"trace_ms": (acc["ms_trace_closest"] + acc["ms_trace_shadow"]) / k, "sort_ms": acc["ms_sort"] / k,
                   "shade_ms": acc["ms_shade"] / k, "camera_ms": acc["ms_camera"] / k, "splat_ms": acc["ms_splat"] / k,
                   "frame_ms": acc["ms_total"] / k, "closest_rays": acc["rays_closest"] // k,
                   "shadow_rays": acc["rays_shadow"] // k,
                   "trace_launches": (acc["launches_trace_closest"] + acc["launches_trace_shadow"]) // k,
                   # tail mode: the paths left at the switch bounce, finished in one k_finish launch
                   "finish_ms": acc["ms_finish"] / k, "finish_paths": acc["paths_finish"] // k,
                   "finish_launches": acc["launches_finish"] // k}
        # counter-backed bandwidth of the other kernels: memory-side bytes of
        # one frame (the committed PMC set of this configuration) / the same
        # set's rocprofv3 kernel time per frame (average duration x launches
        # per frame, so bytes and time come from one profiler on the same
        # kernels; HIP events bracket short kernels loosely, round-3 VERDICT
        # weak #6); this run's HIP-event time is reported beside it
        pj, psrc = pmc_lookup(pmc_key(a, world)) if a.full else (None, None)
        if pj:
            fam_ms = {"k_shade": kernels["shade_ms"], "k_finish": kernels["finish_ms"],
                      "k_camera": kernels["camera_ms"], "k_splat": kernels["splat_ms"]}
            pmc = {}
            for fam, ms in fam_ms.items():
                ks = [v for n, v in pj["kernels"].items() if n == fam or n.startswith(fam + "<")]
                # per frame: the set's pass rendered frames_fetch_pass frames
                # (bench.py --pmc-pass; sets of round 5 and before lack the
                # count and are not quoted)
                if "frames_fetch_pass" not in pj:
                    continue
                b = sum(v.get("traffic_bytes_per_frame", 0.0) for v in ks)
                rp_ns = sum(v["rocprof_stats"]["avg_ns"] * v.get("launches_per_frame", 0) for v in ks
                            if "rocprof_stats" in v)
                if b > 0 and rp_ns > 0:
                    hits = [v["tcc_hit_rate"] for v in ks if "tcc_hit_rate" in v]
                    gbps = b / (rp_ns / 1e9) / 1e9
                    pmc[fam] = {"bytes_per_frame": round(b), "rocprof_ms_per_frame": round(rp_ns / 1e6, 3),
                                "GBps": round(gbps, 1), "frac_of_hbm_peak": round(gbps / HBM_PEAK_GBS, 4),
                                "GBps_hip_events": round(b / (ms / 1e3) / 1e9, 1) if ms > 0 else None,
                                "tcc_hit_rate": hits[0] if len(hits) == 1 else None}
            kernels["pmc"] = pmc
            kernels["pmc_source"] = psrc
    if rank == 0 and a.full and not a.no_count:
        # instrumented pass at reduced spp (per-ray counts are spp-independent)
        pc = params.copy()
        pc.spp = max(1, min(params.spp, 16))
        gpu.set_flags(mtsg.MTSG_FLAG_COUNT)
        mtsg.device_lib().mtsg_device_memset(gpu._h, film, nbytes)
        gpu.render_device(pc, film)
        cs = gpu.stats()
        gpu.set_flags(0)
        per = lambda v, n: v / max(1, n)  # noqa: E731
        nodes_c, tests_c = per(cs.nodes_visited, cs.rays_closest), per(cs.tri_tests, cs.rays_closest)
        nodes_s, tests_s = per(cs.shadow_nodes_visited, cs.rays_shadow), per(cs.shadow_tri_tests, cs.rays_shadow)
        # SURVEY §8(d) algorithmic bytes per ray: 8 B per KDNode visited, 4 B
        # per leaf reference, 48 B per TriAccel test (gkdtree.h:452-480,
        # triaccel.h:37-51), counted by the instrumented pass.  The device
        # layout's own bytes (16 B node pairs, leaf-ordered 48-B records, no
        # index indirection, plus 48 B of ray I/O) are reported beside it.
        refs_c, refs_s = per(cs.leaf_refs, cs.rays_closest), per(cs.shadow_leaf_refs, cs.rays_shadow)
        b_c = 8 * nodes_c + 4 * refs_c + 48 * tests_c
        b_s = 8 * nodes_s + 4 * refs_s + 48 * tests_s
        d_c = 16 * nodes_c + 48 * tests_c + 48
        d_s = 16 * nodes_s + 48 * tests_s + 48
        launches = max(1, acc["launches_trace_closest"] + acc["launches_trace_shadow"])
        trace_s = (acc["ms_trace_closest"] + acc["ms_trace_shadow"]) / 1e3
        bytes_per_launch = (b_c * acc["rays_closest"] + b_s * acc["rays_shadow"]) / launches
        dev_bytes_per_launch = (d_c * acc["rays_closest"] + d_s * acc["rays_shadow"]) / launches
        avg_launch_s = trace_s / launches
        achieved = bytes_per_launch / avg_launch_s / 1e9 if avg_launch_s > 0 else 0.0
        dev_achieved = dev_bytes_per_launch / avg_launch_s / 1e9 if avg_launch_s > 0 else 0.0
        # counters of the same kernel instantiation on the same configuration
        # only (profiles/rNN_pmc_*.json); otherwise null
        tkern = trace_kernel(a)
        pj, psrc = pmc_lookup(pmc_key(a, world))
        tk = (pj or {}).get("kernels", {}).get(tkern, {})
        traffic = None
        if "traffic_bytes_per_launch" in tk and avg_launch_s > 0:
            traffic = round(tk["traffic_bytes_per_launch"] / avg_launch_s / 1e9, 1)
        roofline = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                    "traffic_frac": round(traffic / HBM_PEAK_GBS, 4) if traffic else None,
                    "traffic_source": (f"{psrc} [{tkern}]: FETCH_SIZE x2 + WRITE_SIZE per launch "
                                       f"({tk['traffic_bytes_per_launch'] / 1e9:.2f} GB) / this run's avg launch time; "
                                       "memory-side requests, Infinity-Cache hits included"
                                       if traffic is not None else None),
                    "tcc_hit_rate": tk.get("tcc_hit_rate"),
                    "tcc_source": f"{psrc} [{tkern}]" if "tcc_hit_rate" in tk else None,
                    "kernel": f"{tkern} (closest + shadow rays)",
                    "bytes_model": "SURVEY 8(d): 8 B/KDNode + 4 B/leaf ref + 48 B/TriAccel test",
                    "algorithmic_bytes_per_launch": round(bytes_per_launch), "avg_launch_ms": round(avg_launch_s * 1e3, 3),
                    "launches_per_frame": launches // a.steps,
                    "bytes_per_closest_ray": round(b_c, 1), "bytes_per_shadow_ray": round(b_s, 1),
                    "device_layout": {"achieved": round(dev_achieved, 1), "frac": round(dev_achieved / HBM_PEAK_GBS, 4),
                                      "bytes_per_closest_ray": round(d_c, 1), "bytes_per_shadow_ray": round(d_s, 1),
                                      "model": "16 B node pair per inner node + 48 B leaf-ordered TriAccel per test + 48 B ray I/O"},
                    "nodes_per_closest_ray": round(nodes_c, 2), "tests_per_closest_ray": round(tests_c, 2),
                    "nodes_per_shadow_ray": round(nodes_s, 2), "tests_per_shadow_ray": round(tests_s, 2),
                    # SIMD efficiency of the traversal waves (instrumented pass)
                    "simd_active_lanes": round(per(cs.wave_active_lanes, 64 * cs.wave_steps), 3),
                    "simd_eff_inner": round(per(cs.nodes_visited + cs.shadow_nodes_visited, 64 * cs.wave_node_iters), 3),
                    "simd_eff_leaf": round(per(cs.tri_tests + cs.shadow_tri_tests, 64 * cs.wave_test_iters), 3),
                    # lane-iterations of the traversal loop per ray (one node
                    # fetch + one primitive fetch each), and instance entries
                    "iterations_per_ray": round(per(cs.wave_active_lanes, cs.rays_closest + cs.rays_shadow), 2),
                    "instance_visits_per_ray": round(per(cs.instance_visits + cs.shadow_instance_visits,
                                                         cs.rays_closest + cs.rays_shadow), 3),
                    # entries whose group-box clip left an empty interval
                    "instance_entries_rejected": round(per(cs.instance_rejects,
                                                           cs.instance_visits + cs.shadow_instance_visits), 3),
                    # instance primitives the world-box prefilter skipped, per ray
                    "instance_prefiltered_per_ray": round(per(cs.instance_prefiltered,
                                                              cs.rays_closest + cs.rays_shadow), 3),
                    # the exactness paths (flattened traversal): exact-tie
                    # retraces with the mailbox (k_tie) and the restart
                    # guard's one-ulp steps, in the instrumented pass and
                    # scaled to one frame at the run's spp
                    "exactness_paths": {
                        "count_pass_spp": int(pc.spp),
                        "tie_retraces": int(cs.tie_retraces),
                        "tie_retraces_per_frame": round(cs.tie_retraces * params.spp / pc.spp),
                        "kd_restarts_closest": int(cs.restarts_closest), "kd_restarts_shadow": int(cs.restarts_shadow),
                        "guard_rays_closest": int(cs.guard_rays_closest), "guard_rays_shadow": int(cs.guard_rays_shadow),
                        "guard_steps_closest": int(cs.guard_steps_closest),
                        "guard_steps_shadow": int(cs.guard_steps_shadow),
                        "guard_rays_per_frame": round((cs.guard_rays_closest + cs.guard_rays_shadow)
                                                      * params.spp / pc.spp),
                        "scope": ("flattened traversal" if a.instancing == "flatten"
                                  else "two-level: not counted (per-level restart counters)")}}

    # the host-side tile gather: every rank's share of the timed steps' last
    # frame into rank 0's ImageBlock (after the timed region)
    frame = assembly = parity = None
    if not emulated:
        nw = windows_for(params)
        keys = None if cur["keys"] is None else cur["keys"].copy()
        part = ("win", host_win[:nw[0]].copy(), keys) if nw else ("block", host_block.copy(), None)
        frame = gather_frame(pg, rank, world, part, params.tile_w, params.tile_h, border)
    if rank == 0 and a.dump_outputs:
        # what a caller of the timed path receives: the frame's ImageBlock
        # (with emulated shares: the whole frame of the last whole-frame step)
        os.makedirs(a.dump_outputs, exist_ok=True)
        np.save(os.path.join(a.dump_outputs, "imageblock.npy"),
                np.ascontiguousarray(host_block if frame is None else frame, dtype=np.float32))
    use_whole()
    if rank == 0 and world > 1 and a.full:
        # the assembled frame vs the whole frame rendered by rank 0's GPU alone
        # (global RNG keys: the same samples; the film's float additions may
        # run in another order)
        pw = params.copy()
        pw.tile_stride, pw.tile_offset = 1, 0
        mtsg.device_lib().mtsg_device_memset(gpu._h, film, nbytes)
        gpu.render_device(pw, film)
        whole = gpu.download(film, (H, W, 5))
        diff = np.abs(frame - whole)
        assembly = {"check": f"frame assembled from {world} ranks' tile ImageBlocks vs the whole frame rendered on rank 0's GPU",
                    "max_abs_diff": float(diff.max()), "max_value": float(np.abs(whole).max()),
                    "pass": bool(np.allclose(frame, whole, rtol=1e-5, atol=1e-6)),
                    "tiles_per_rank": counts.tolist()}
    if rank == 0 and a.save and frame is not None:
        np.save(a.save, mtsg.develop(frame[border:H - border, border:W - border]))
    if rank == 0 and frame is not None and a.full and not a.no_parity:
        parity = parity_at_headline(scene, frame, params, border, a.parity_stride, world)
    cpu = None
    if rank == 0 and world == 1 and a.full and not a.no_cpu:
        cpu = cpu_baseline(scene, params, border, a.cpu_seconds)

    gpu.free(film)
    if wbuf is not None:
        gpu.free(wbuf)
    gpu.close()
    if rank == 0:
        out = {
            "metric": "Msamples/sec at 1280x720x256spp, 1/2/4/8 MI355X; per-pixel L1 vs CPU ref",
            "value": round(value, 3), "unit": "Msamples/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(ms_per_step, 2), "higher_is_better": True, "scaling": "strong",
            **({"devices": devices} if devices else {}),
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": {"bunny15": ("C3 bunny x15, 1,041,765 triangles, roughconductor Cu GGX 0.2" + (
                                        ", 15 instances flattened to world-space triangles" if a.instancing == "flatten" else "")),
                                    "cbox": "C2 Cornell box, diffuse + area emitter",
                                    "c5": "C5 dielectric + roughconductor bunnies under data/tests/envmap.exr (HDR envmap), maxDepth 64"}[a.workload]
                       + (" [two-level: 15 instances of one 69,451-triangle shapegroup, Mitsuba's instance.cpp structure]"
                          if a.instancing == "two-level" and a.workload == "bunny15" else ""),
                       "resolution": f"{params.tile_w}x{params.tile_h}", "spp": params.spp,
                       "max_depth": 64 if a.workload == "c5" else 8,
                       "samples_per_step": params.tile_w * params.tile_h * params.spp,
                       "parallelism": f"film tiles round-robin over {world} GPU(s)",
                       "scene_load_s": round(load_s, 2), **kd_info},
            **({"emulated_ranks": a.emulate_ranks,
                "share_ms_per_step": [round(t / a.steps * 1e3, 3) for t in share_s],
                "whole_frame_ms_per_step": round(whole_s / a.steps * 1e3, 3) if whole_s else None,
                "share_speedups": [round(whole_s / t, 3) for t in share_s] if whole_s else None,
                "share_speedup_min": round(whole_s / max(share_s), 3) if whole_s else None,
                "note": "one GPU rendering each rank's tile share in turn; value = frame samples / the slowest "
                        "share's time (the N-GPU frame time without launch and gather overheads); kernels = share 0"}
               if a.emulate_ranks > 1 and world == 1 else {}),
            **({"balance": {"rounds": balance_log, "tiles_per_share": counts.tolist(),
                            "layout": a.share_layout,
                            "method": "shares are runs of the golden-ratio key order (mtsg.balance_order; "
                                      "--share-layout bands: the row-major key order); each "
                                      "warm-up round times every share (the faster of two steps) and gives share r "
                                      "tiles in proportion to its measured rate, damped 1/2 (mtsg.balance_cuts); "
                                      "the timed steps use the last cut"}}
               if balanced else {}),
            "roofline": roofline, "cpu_baseline": cpu, "parity": parity,
            **({"assembly": assembly} if assembly else {}), "kernels": kernels,
        }
        print(json.dumps(out))
    if pg is not None:
        barrier(pg)   # the other ranks wait for rank 0's checks
        pg.destroy_process_group()


if __name__ == "__main__":
    main()
