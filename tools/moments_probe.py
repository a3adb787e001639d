#!/usr/bin/env python3
"""Measurements of the per-pixel sample moments (rpt_set_moments, rpt_noise_count, rpt_render_to_noise; csrc/k_moments.h, csrc/k_complete.h).

  python tools/moments_probe.py --cpu                 no GPU: the `above` counts of the numpy restatement (tests/moments_ref.py) over the CPU oracle's samples at
                                                      100 x 70 — VeachMIS nee 1, DarkCornell nee 1 and nee 0, every 8 samples up to 128 (DESIGN.md "Moments and noise estimate")
  python tools/moments_probe.py --cost [workload ..]  one MI355X: moments off and on ALTERNATED in one process, 32-spp batches.  Pass 1: the whole-batch time (host
                                                      clock around rpt_render, which synchronises).  Pass 2, a context with RPT_STAGE_TIMING=1 (events between the
                                                      stage kernels slow the batch: never the same pass as the batch times): kernel_ms[RPT_STAGE_COMPLETE] per batch.
                                                      Then one image each way from the same seeds: the accumulator words that differ (must be 0).
  python tools/moments_probe.py --target              one MI355X: VeachMIS 1080p MIS, rpt_render_to_noise(threshold 0.1, max_above 1 % of the pixels, batches of 32,
                                                      at most 1024): samples rendered, ms, and the ms outside rendering = that minus the same number of 32-spp
                                                      batches rendered plainly with moments on (median of 3); and the count kernel alone (median of 25 calls).
Workloads of --cost: darkcornell (DarkCornell 1024^2) and pbrtest (PBRTest 2048^2), bench.py's configurations of the same names.  Output goes to stdout
(kept in profiles/r12_moments.txt).  Needs the GPU for --cost / --target: there is no fallback."""
import argparse
import importlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

try:
    import torch  # noqa: F401  (first: see tests/conftest.py)
except ImportError:
    pass
import numpy as np  # noqa: E402

WORKLOADS = {"darkcornell": ("DarkCornell", 1024, 1024, {}), "pbrtest": ("PBRTest", 2048, 2048, {}), "veachmis": ("VeachMIS", 1920, 1080, {"nee": 1})}


def spread(xs):
    return f"median {statistics.median(xs):8.3f}  min {min(xs):8.3f}  max {max(xs):8.3f}  ({len(xs)} batches)"


def cpu():
    from oracle_ffi import Oracle
    import moments_ref as ref
    rpt = importlib.import_module("rust-path-tracer_amd")
    orc = Oracle("rpt_math")
    W, H = 100, 70
    for scene, nee, thresholds in (("VeachMIS", 1, (0.05, 0.1, 0.3)), ("DarkCornell", 1, (0.1, 0.2, 0.3)), ("DarkCornell", 0, (0.1, 0.2, 0.3))):
        bank = ref.SampleBank(orc, rpt.default_config(W, H, nee=nee), rpt.World.from_path(rpt.fixture(scene + ".glb")), rpt.blue_noise_seeds(W, H))
        print(f"{scene} nee {nee}, {W} x {H} = {W * H} pixels: samples | above " + " / ".join(f"{t:g}" for t in thresholds) + " | zero variance")
        m = np.zeros((H, W, 4), np.float32)
        for n in range(1, 129):
            bank.need(n)
            ref.add_sample(m, bank.radiance[n - 1])
            if n % 8 == 0:
                rel = ref.noise_rel(m)
                print(f"  {n:4d} | " + " / ".join(str(ref.noise_counts(m, t)["above"]) for t in thresholds) + f" | {int((rel == 0).sum())}")


def timed_pass(hip, world, cfg, seeds, spp, warmup, batches, stage_timing):
    """{off / on: [ms per batch]}: host clock around rpt_render, or the completion stage's HIP-event time with RPT_STAGE_TIMING=1"""
    if stage_timing:
        os.environ["RPT_STAGE_TIMING"] = "1"
    else:
        os.environ.pop("RPT_STAGE_TIMING", None)
    r = hip.Renderer(0)
    out = {"off": [], "on": []}
    try:
        r.upload_scene(world)
        r.set_config(cfg)
        r.reset(seeds)
        for k in range(warmup + batches):
            for mode in ("off", "on"):
                r.set_moments(mode == "on")
                before = r.stats()["kernel_ms"]["complete"] if stage_timing else 0.0
                t0 = time.perf_counter()
                r.render(spp)
                ms = (time.perf_counter() - t0) * 1e3
                if stage_timing:
                    ms = r.stats()["kernel_ms"]["complete"] - before
                if k >= warmup:
                    out[mode].append(ms)
    finally:
        r.close()
        os.environ.pop("RPT_STAGE_TIMING", None)
    return out


def cost(names, spp, warmup, batches):
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    print(f"# library {hip.lib_path()} (sources {hip.build_fingerprint()}); {batches} timed batches of {spp} spp each way after {warmup} warm-up, off / on alternate")
    for name in names:
        scene, W, H, over = WORKLOADS[name]
        world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
        cfg = rpt.default_config(W, H, **over)
        seeds = rpt.blue_noise_seeds(W, H)
        batch = timed_pass(hip, world, cfg, seeds, spp, warmup, batches, False)
        stage = timed_pass(hip, world, cfg, seeds, spp, warmup, batches, True)
        images = {}
        r = hip.Renderer(0)
        try:
            r.upload_scene(world)
            r.set_config(cfg)
            for mode in ("off", "on"):
                r.set_moments(mode == "on")
                r.reset(seeds)
                r.render(spp)
                images[mode] = r.read_accum()[0].copy()
            mz = r.read_moments()[..., 2]
        finally:
            r.close()
        print(f"{name}: {scene} {W}x{H}")
        for mode in ("off", "on"):
            print(f"  moments {mode:3s} batch ms            {spread(batch[mode])}")
            print(f"  moments {mode:3s} completion stage ms {spread(stage[mode])}   [separate pass, RPT_STAGE_TIMING=1]")
        b0, b1 = statistics.median(batch["off"]), statistics.median(batch["on"])
        s0, s1 = statistics.median(stage["off"]), statistics.median(stage["on"])
        print(f"  on vs off: batch {100 * (b1 / b0 - 1):+.2f} %, completion stage {100 * (s1 / s0 - 1):+.1f} % ({s0:.3f} -> {s1:.3f} ms = {100 * s0 / b0:.1f} % -> {100 * s1 / b0:.1f} % of the batch); "
              f"accumulator words that differ: {int((images['off'].view(np.uint32) != images['on'].view(np.uint32)).sum())} of {images['off'].size}; m.z == {spp} everywhere: {bool((mz == spp).all())}")
        sys.stdout.flush()


def target():
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    scene, W, H, over = WORKLOADS["veachmis"]
    world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
    cfg = rpt.default_config(W, H, **over)
    seeds = rpt.blue_noise_seeds(W, H)
    threshold, max_above = 0.1, W * H // 100
    r = hip.Renderer(0)
    try:
        r.upload_scene(world)
        r.set_config(cfg)
        r.reset(seeds)
        r.set_moments(True)
        r.render(32)                                     # warm-up (allocations, clocks)
        r.reset(seeds)
        res = r.render_to_noise(threshold, max_above=max_above, batch_samples=32, min_samples=32, max_samples=1024)
        image = r.read_accum()[0].copy()
        count_ms = []
        for _ in range(25):
            t0 = time.perf_counter()
            r.noise_count(threshold)
            count_ms.append((time.perf_counter() - t0) * 1e3)
        plain = []
        n_batches = res["samples_rendered"] // 32
        for _ in range(3):
            r.reset(seeds)
            t0 = time.perf_counter()
            for _ in range(n_batches):
                r.render_async(32)
            r.wait()
            plain.append((time.perf_counter() - t0) * 1e3)
        same = bool(np.array_equal(r.read_accum()[0].view(np.uint32), image.view(np.uint32)))
    finally:
        r.close()
    p = statistics.median(plain)
    print(f"# library {hip.lib_path()} (sources {hip.build_fingerprint()})")
    print(f"veachmis: {scene} {W}x{H} MIS, rpt_render_to_noise(threshold {threshold}, max_above {max_above} = 1 % of the pixels, batches of 32, min 32, max 1024)")
    print(f"  samples rendered {res['samples_rendered']}, converged {res['converged']}, counts {res['counts']}, {res['ms']:.2f} ms")
    print(f"  the same {n_batches} batches rendered plainly (moments on, asynchronous, one wait): median {p:.2f} ms (min {min(plain):.2f}, max {max(plain):.2f}); "
          f"outside rendering: {res['ms'] - p:.2f} ms = {(res['ms'] - p) / max(n_batches, 1):.3f} ms per batch; accumulator bit for bit the same: {same}")
    print(f"  rpt_noise_count alone (kernel + wait + 24-byte read-back, host clock): {spread(count_ms)}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--cost", nargs="*", default=None, metavar="WORKLOAD")
    ap.add_argument("--target", action="store_true")
    ap.add_argument("--spp", type=int, default=32)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.cpu:
        cpu()
    if args.cost is not None:
        cost(args.cost or ["darkcornell", "pbrtest"], args.spp, args.warmup, args.batches)
    if args.target:
        target()
    if not (args.cpu or args.cost is not None or args.target):
        print(__doc__)
