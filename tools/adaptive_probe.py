#!/usr/bin/env python3
"""What per-pixel sample counts save over stopping the whole image (rpt_render_adaptive against rpt_render_to_noise; csrc/k_adaptive.h, rpt_adaptive.hip).

  python tools/adaptive_probe.py --cpu                     no GPU: from tests/moments_ref.py SampleBank alone (the CPU oracle's per-sample radiances, 100 x 70, nee 1,
                                                           blue-noise seeds), the per-pixel counts and the total pixel-samples of a target under uniform stopping
                                                           (rpt_render_to_noise) and under adaptive stopping (rpt_render_adaptive), VeachMIS and DarkCornell.  Exact
                                                           predictions: tests/test_gpu_adaptive.py holds the device to the adaptive ones.
  python tools/adaptive_probe.py --gpu --parent-lib PATH   one MI355X: DarkCornell 1024^2 MIS and VeachMIS 1080p MIS, the same target both ways, ONE PROCESS PER LEG,
                                                           each under its own `timeout`: the uniform leg is rpt_render_to_noise with the library at PATH (a build of the
                                                           parent commit, through RPT_HIP_LIB), the adaptive leg rpt_render_adaptive with the in-tree library.  Reports ms,
                                                           pixel-samples, passes, and the masked passes' Grays/s against the whole-image rate of the same process.
  (--leg uniform|adaptive WORKLOAD: what --gpu starts; prints one line.)
Output goes to stdout (kept in profiles/r13_adaptive.txt).  There is no fallback: --gpu needs the GPU."""
import argparse
import importlib
import json
import os
import subprocess
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

WORKLOADS = {"darkcornell_mis": ("DarkCornell", 1024, 1024), "veachmis": ("VeachMIS", 1920, 1080)}
# the device target: noise at or below 0.1 for all but 1 % of the pixels, 16 samples at a time, at most 256
GPU_TARGET = dict(threshold=0.1, batch_samples=16, min_samples=16, max_samples=256)
CPU_TARGETS = (("VeachMIS", 0.3, 0, 64), ("VeachMIS", 0.3, 43, 128), ("DarkCornell", 0.2, 0, 64), ("DarkCornell", 0.2, 350, 64))


def cpu():
    from oracle_ffi import Oracle
    import adaptive_ref as aref
    import moments_ref as ref
    rpt = importlib.import_module("rust-path-tracer_amd")
    orc = Oracle("rpt_math")
    W, H = 100, 70
    banks = {}
    for scene, threshold, max_above, cap in CPU_TARGETS:
        if scene not in banks:
            banks[scene] = ref.SampleBank(orc, rpt.default_config(W, H, nee=1), rpt.World.from_path(rpt.fixture(scene + ".glb")), rpt.blue_noise_seeds(W, H))
        b, t = banks[scene], aref.Target(threshold, max_above, 8, 8, cap)
        n_uniform, conv_uniform = aref.uniform_stop(b, t)
        sim = aref.simulate(b, t)
        counts, pixels = np.unique(sim["counts_image"], return_counts=True)
        print(f"{scene} nee 1, {W} x {H} = {W * H} pixels, threshold {threshold:g}, at most {max_above} above, min 8, batches of 8, max {cap}")
        print(f"  uniform stopping   {n_uniform:4d} samples on every pixel, converged {conv_uniform}: {n_uniform * W * H} pixel-samples, "
              f"above at the end {ref.noise_counts(b.moments(n_uniform), threshold)['above']}")
        print(f"  adaptive stopping  {sim['passes']} masked passes, converged {sim['converged']}: {sim['pixel_samples']} pixel-samples "
              f"({100.0 * sim['pixel_samples'] / (n_uniform * W * H):.1f} % of uniform), above at the end {sim['counts']['above']}")
        print("  pixels per final count: " + ", ".join(f"{int(c)}: {int(p)}" for c, p in zip(counts, pixels)))


def leg(kind, workload):
    """one leg in this process: {"ms", "pixel_samples", ...} as one JSON line"""
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    scene, W, H = WORKLOADS[workload]
    world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
    cfg, seeds = rpt.default_config(W, H, nee=1), rpt.blue_noise_seeds(W, H)
    target = dict(GPU_TARGET, max_above=W * H // 100)
    r = hip.Renderer(0)
    try:
        r.upload_scene(world)
        r.set_config(cfg)
        r.reset(seeds)
        r.set_moments(True)
        r.render(target["batch_samples"])                    # warm-up (allocations, clocks)
        out = {"leg": kind, "workload": workload, "library": hip.lib_path(), "sources": hip.build_fingerprint()}

        def rays():
            st = r.stats()
            return st["extension_rays"] + st["shadow_rays_traced"]

        # the whole-image rate of this process: the uniform phase alone
        r.reset(seeds)
        t0 = time.perf_counter()
        for _ in range(target["min_samples"] // target["batch_samples"]):
            r.render_async(target["batch_samples"])
        r.wait()
        whole_ms, whole_rays = (time.perf_counter() - t0) * 1e3, rays()
        out["whole_image_grays_per_s"] = whole_rays / whole_ms / 1e6
        r.reset(seeds)
        if kind == "uniform":
            res = r.render_to_noise(**target)
            out.update(ms=res["ms"], pixel_samples=res["samples_rendered"] * W * H, samples=res["samples_rendered"], converged=res["converged"], counts=res["counts"])
        else:
            res = r.render_adaptive(**target)
            masked_ms, masked_rays = res["ms"] - whole_ms, rays() - whole_rays
            out.update(ms=res["ms"], pixel_samples=res["pixel_samples"], passes=res["passes"], converged=res["converged"], counts=res["counts"],
                       min_pixel_samples=res["min_pixel_samples"], max_pixel_samples=res["max_pixel_samples"],
                       masked_passes_grays_per_s=(masked_rays / masked_ms / 1e6) if res["passes"] and masked_ms > 0 else None)
        out["grays_per_s"] = rays() / out["ms"] / 1e6
    finally:
        r.close()
    print(json.dumps(out))


def gpu(parent_lib, names, limit):
    if not parent_lib or not os.path.exists(parent_lib):
        sys.exit("--gpu needs --parent-lib: librpt_hip.so built from the parent commit (the uniform leg is measured against it)")
    print(f"# target {GPU_TARGET}, max_above = 1 % of the pixels; uniform leg: rpt_render_to_noise, library {parent_lib}; adaptive leg: rpt_render_adaptive, in-tree library")
    for name in names:
        for kind in ("uniform", "adaptive"):
            env = dict(os.environ)
            env.pop("RPT_HIP_LIB", None)
            if kind == "uniform":
                env["RPT_HIP_LIB"] = os.path.abspath(parent_lib)
            done = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", kind, name], env=env, capture_output=True, text=True)
            if done.returncode != 0:                         # a leg that failed ends the run: nothing more is started on the GPU
                sys.exit(f"{name} {kind}: exit status {done.returncode}\n{done.stdout}{done.stderr}")
            print(f"{name} {kind}: {done.stdout.strip().splitlines()[-1]}")
            sys.stdout.flush()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--workloads", nargs="*", default=list(WORKLOADS))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per leg")
    ap.add_argument("--leg", nargs=2, metavar=("KIND", "WORKLOAD"))
    args = ap.parse_args()
    if args.cpu:
        cpu()
    if args.gpu:
        gpu(args.parent_lib, args.workloads, args.timeout)
    if args.leg:
        leg(*args.leg)
    if not (args.cpu or args.gpu or args.leg):
        print(__doc__)
