#!/usr/bin/env python3
"""What RPT_SHADOW_SEGMENT (rpt.h rpt_set_shadow_mode) is worth on the device, and what it changes: A/B of the two shadow modes in ONE process.

usage: python tools/shadow_mode_ab.py [workload ...] [--batches K] [--warmup W] [--spp 32] [--modes exact,segment]
Workloads are bench.py's configurations: darkcornell_mis (DarkCornell 1024^2), veachmis (VeachMIS 1080p), deepbvh (the 1 M-triangle stand-in, 2048^2), all nee = MIS.

Per workload: one context; W warm-up batches per mode, then K timed batches of --spp samples in each mode ALTERNATELY (exact, segment, exact, ... — drift of the
clocks hits both alike); the batch time is the host clock around rpt_render, which synchronises.  A second context with RPT_STAGE_TIMING=1 (HIP events between
the stage kernels slow the batch: never the same pass as the batch times) gives kernel_ms[RPT_STAGE_SHADOW] per batch the same way.  Then one image per mode from
the same seeds: the accumulator words that differ.  Reported per mode: median, min, max of the repeats.
With RPT_HIP_LIB naming a build from before the mode existed only the exact leg runs (the yardstick that is not the code under test).
Needs the GPU: there is no fallback."""
import argparse
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

try:
    import torch  # noqa: F401  (first: see tests/conftest.py)
except ImportError:
    pass
import numpy as np  # noqa: E402

WORKLOADS = {
    # bench.py WORKLOADS of the same names
    "darkcornell_mis": ("DarkCornell", 1024, 1024, {"nee": 1}),
    "veachmis": ("VeachMIS", 1920, 1080, {"nee": 1}),
    "deepbvh": ("procedural:deep_bvh_1M", 2048, 2048, {"nee": 1, "cam_position": (0.0, 2.5, -0.5, 0.0)}),
}
MODES = {"exact": 0, "segment": 1}


def load_world(rpt, scene):
    if scene == "procedural:deep_bvh_1M":
        from scenes import deep_bvh_scene
        return deep_bvh_scene(1_000_000)
    return rpt.World.from_path(rpt.fixture(scene + ".glb"))


def spread(xs):
    return f"median {statistics.median(xs):8.3f}  min {min(xs):8.3f}  max {max(xs):8.3f}  ({len(xs)} batches)"


def timed_pass(hip, world, cfg, seeds, modes, spp, warmup, batches, stage_timing):
    """{mode: [ms per batch]}: host clock around rpt_render, or the shadow stage's HIP-event time with RPT_STAGE_TIMING=1"""
    if stage_timing:
        os.environ["RPT_STAGE_TIMING"] = "1"
    else:
        os.environ.pop("RPT_STAGE_TIMING", None)
    r = hip.Renderer(0)
    out = {m: [] for m in modes}
    try:
        r.upload_scene(world)
        r.set_config(cfg)
        r.reset(seeds)
        for k in range(warmup + batches):
            for m in modes:
                if len(modes) > 1 or m != "exact":
                    r.set_shadow_mode(MODES[m])
                before = r.stats()["kernel_ms"]["shadow"] if stage_timing else 0.0
                t0 = time.perf_counter()
                r.render(spp)
                ms = (time.perf_counter() - t0) * 1e3
                if stage_timing:
                    ms = r.stats()["kernel_ms"]["shadow"] - before
                if k >= warmup:
                    out[m].append(ms)
    finally:
        r.close()
        os.environ.pop("RPT_STAGE_TIMING", None)
    return out


def images(hip, world, cfg, seeds, modes, spp):
    r = hip.Renderer(0)
    out = {}
    try:
        r.upload_scene(world)
        r.set_config(cfg)
        for m in modes:
            if len(modes) > 1 or m != "exact":
                r.set_shadow_mode(MODES[m])
            r.reset(seeds)
            r.render(spp)
            out[m] = (r.read_accum()[0].copy(), r.stats())
    finally:
        r.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workloads", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--modes", default="exact,segment")
    args = ap.parse_args()
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    modes = [m for m in args.modes.split(",") if m]
    assert all(m in MODES for m in modes), modes
    if not hasattr(hip.lib(), "rpt_set_shadow_mode"):
        print(f"# {hip.lib_path()} has no rpt_set_shadow_mode: the exact leg only")
        modes = ["exact"]
    print(f"# library {hip.lib_path()} (sources {hip.build_fingerprint()}); {args.batches} timed batches of {args.spp} spp per mode after {args.warmup} warm-up, modes alternate")
    for name in args.workloads:
        scene, W, H, over = WORKLOADS[name]
        world = load_world(rpt, scene)
        cfg = rpt.default_config(W, H, **over)
        seeds = rpt.blue_noise_seeds(W, H)
        batch = timed_pass(hip, world, cfg, seeds, modes, args.spp, args.warmup, args.batches, False)
        stage = timed_pass(hip, world, cfg, seeds, modes, args.spp, args.warmup, args.batches, True)
        img = images(hip, world, cfg, seeds, modes, args.spp)
        print(f"{name}: {scene} {W}x{H} nee = MIS")
        for m in modes:
            st = img[m][1]
            print(f"  {m:8s} batch ms        {spread(batch[m])}")
            print(f"  {m:8s} shadow stage ms {spread(stage[m])}   [separate pass, RPT_STAGE_TIMING=1]")
            print(f"  {m:8s} shadow rays {st['shadow_rays']} (elided {st['shadow_rays_elided']}), extension rays {st['extension_rays']}")
        if len(modes) == 2:
            a, b = img[modes[0]][0], img[modes[1]][0]
            e, s = statistics.median(batch[modes[0]]), statistics.median(batch[modes[1]])
            es, ss = statistics.median(stage[modes[0]]), statistics.median(stage[modes[1]])
            print(f"  {modes[1]} vs {modes[0]}: batch {100 * (s / e - 1):+.1f} %, shadow stage {100 * (ss / es - 1):+.1f} %; "
                  f"accumulator words that differ: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} of {a.size}")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
