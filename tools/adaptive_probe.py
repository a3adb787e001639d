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
  python tools/adaptive_probe.py --cpu-window [--sizes 100x70 200x140]
                                                           no GPU: the window rule of rpt_render_adaptive_window (a pixel is sampled while any pixel of its window is
                                                           noisy) for radius 0 .. 3 on DarkCornell without and with NEE and VeachMIS: pixel-samples, passes, pixels stopped
                                                           at min_samples, energy and rel-L2 against an independent converged image, and a uniform image of equal budget
                                                           (kept in profiles/r17_adaptive_window_quality.txt; hip.ADAPTIVE_WINDOW_RADIUS is its minimum).
  python tools/adaptive_probe.py --gpu-window              one MI355X, the same two workloads, one process each under its own `timeout`: the selection step alone at radius
                                                           0, 1, 3 and 8 (HIP events, median of 25) beside the masked pass it precedes, and rpt_render_adaptive against
                                                           rpt_render_adaptive_window at the recommended radius (kept in profiles/r17_adaptive_window.txt).
  (--window-leg WORKLOAD: what --gpu-window starts; prints one line.)
Output goes to stdout (--cpu, --gpu: kept in profiles/r13_adaptive.txt).  There is no fallback: --gpu and --gpu-window need the GPU."""
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


WINDOW_CONFIGS = (("DarkCornell", 0, 0.2), ("DarkCornell", 1, 0.2), ("VeachMIS", 1, 0.3))
WINDOW_RADII = (0, 1, 2, 3)
WINDOW_TARGET = dict(max_above=0, batch_samples=8, min_samples=8, max_samples=128)
WINDOW_REFERENCE_SAMPLES = 2048


def cpu_window(sizes):
    """what the window rule of rpt_render_adaptive_window buys, from the CPU oracle alone: per configuration and radius the pass-by-pass prediction
    (tests/adaptive_window_ref.py simulate), its image against an independent converged one — WINDOW_REFERENCE_SAMPLES FURTHER samples of the same sequence,
    none of which the adaptive image used — and the uniform image of the same budget (the nearest whole sample count)."""
    from oracle_ffi import Oracle
    import adaptive_ref as aref
    import adaptive_window_ref as awr
    import moments_ref as ref
    rpt = importlib.import_module("rust-path-tracer_amd")
    orc = Oracle("rpt_math")
    t = aref.Target(0.0, **WINDOW_TARGET)
    print(f"# window rule on the CPU oracle: min {t.min_samples}, batches of {t.batch_samples}, cap {t.max_samples}, max_above {t.max_above}, blue-noise seeds; reference = "
          f"{WINDOW_REFERENCE_SAMPLES} further samples of the same sequence; energy = summed radiance over the reference's; uniform = every pixel the nearest whole "
          f"number of samples to the adaptive image's mean")
    summed = {}
    for W, H in sizes:
        for scene, nee, threshold in WINDOW_CONFIGS:
            cfg = rpt.default_config(W, H, nee=nee)
            b = ref.SampleBank(orc, cfg, rpt.World.from_path(rpt.fixture(scene + ".glb")), rpt.blue_noise_seeds(W, H))
            b.need(t.max_samples)
            want = orc.trace_cpu(cfg, b.scene, b.rng(t.max_samples), WINDOW_REFERENCE_SAMPLES)[0][..., :3].astype(np.float64) / WINDOW_REFERENCE_SAMPLES
            t.threshold = threshold

            def against(image):
                image = image.astype(np.float64)
                return image.sum() / want.sum(), float(np.linalg.norm(image - want) / np.linalg.norm(want))

            print(f"{scene}/nee{nee} {W} x {H} = {W * H} pixels, threshold {threshold:g}")
            for radius in WINDOW_RADII:
                sim = awr.simulate(b, t, radius)
                n = sim["counts_image"]
                acc = aref.expected_state(b, n)[0]
                energy, err = against(acc[..., :3] / acc[..., 3:4])
                spp = sim["pixel_samples"] / (W * H)
                n_uniform = max(1, int(round(spp)))
                u_energy, u_err = against(b.accum(n_uniform)[..., :3] / np.float32(n_uniform))
                print(f"  radius {radius}: {sim['pixel_samples']:9d} pixel-samples ({spp:6.1f} per pixel), {sim['passes']:2d} passes, converged {sim['converged']}, "
                      f"{int((n == t.min_samples).sum()):6d} pixels stopped at {t.min_samples}, energy {energy:.3f}, rel-L2 {err:.3f} | uniform {n_uniform:3d} spp: energy {u_energy:.3f}, "
                      f"rel-L2 {u_err:.3f}")
                sys.stdout.flush()
                key = (W, H, radius)
                s = summed.setdefault(key, [0.0, 0.0, 0])
                s[0] += err; s[1] += u_err; s[2] += sim["pixel_samples"]
    for W, H in sizes:
        print(f"grid {W} x {H} (summed over the {len(WINDOW_CONFIGS)} configurations): radius | rel-L2 | rel-L2 of the uniform images of equal budget | pixel-samples")
        for radius in WINDOW_RADII:
            s = summed[(W, H, radius)]
            print(f"{radius} | {s[0]:.4f} | {s[1]:.4f} | {s[2]}")


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


def window_leg(workload):
    """one workload in this process, as one JSON line: per radius the selection step alone (HIP events around the select kernels, rpt_debug_adaptive_select_ms:
    median and least of 25, after 16 uniform samples) beside the masked pass that selection precedes (host clock over render_pixels(its mask, batch) up to
    the wait), then the whole calls: render_adaptive against render_adaptive_window at the recommended radius, same target, same seeds"""
    import ctypes as C
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    scene, W, H = WORKLOADS[workload]
    world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
    cfg, seeds = rpt.default_config(W, H, nee=1), rpt.blue_noise_seeds(W, H)
    target = dict(GPU_TARGET, max_above=W * H // 100)
    t = hip.NoiseTarget(target["threshold"], target["min_samples"], target["max_samples"], target["batch_samples"], target["max_above"])
    out = {"workload": workload, "pixels": W * H, "target": target, "sources": hip.build_fingerprint(), "select": {}}
    r = hip.Renderer(0)
    try:
        r.upload_scene(world)
        r.set_config(cfg)
        r.reset(seeds)
        r.set_moments(True)
        r.render(target["batch_samples"])                    # warm-up (allocations, clocks)
        for radius in (0, 1, 3, 8):
            r.reset(seeds)
            r.render(target["min_samples"])
            ms = np.zeros(25, np.float32)
            r._check(hip.lib().rpt_debug_adaptive_select_ms(r._h, C.byref(t), radius, len(ms), hip.ptr(ms)))
            mask, counts = r.adaptive_mask(radius, **target)
            t0 = time.perf_counter()
            r.render_pixels(mask, target["batch_samples"])
            r.wait()
            pass_ms = (time.perf_counter() - t0) * 1e3
            out["select"][radius] = {"select_ms_median": float(np.median(ms)), "select_ms_min": float(ms.min()), "selected": int(mask.sum()), "above": counts["above"],
                                     "pass_ms": pass_ms, "select_over_pass": float(np.median(ms)) / pass_ms}
        for name, call in (("render_adaptive", lambda: r.render_adaptive(**target)),
                           ("render_adaptive_window", lambda: r.render_adaptive_window(hip.ADAPTIVE_WINDOW_RADIUS, **target))):
            r.reset(seeds)
            res = call()
            out[name] = {k: res[k] for k in ("ms", "pixel_samples", "passes", "converged", "min_pixel_samples", "max_pixel_samples", "counts")}
        out["radius"] = hip.ADAPTIVE_WINDOW_RADIUS
    finally:
        r.close()
    print(json.dumps(out))


def gpu_window(names, limit):
    print(f"# window rule on the device: target {GPU_TARGET}, max_above = 1 % of the pixels; one process per workload; select = HIP events around the select kernels, "
          f"radius 0 = the kernels of rpt_render_adaptive (k_ad_count<AdNoiseSel>, k_ad_scan), radius > 0 = k_ad_window, k_ad_count<AdFlagSel>, k_ad_scan")
    for name in names:
        done = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--window-leg", name], capture_output=True, text=True)
        if done.returncode != 0:                             # a leg that failed ends the run: nothing more is started on the GPU
            sys.exit(f"{name}: exit status {done.returncode}\n{done.stdout}{done.stderr}")
        print(f"{name}: {done.stdout.strip().splitlines()[-1]}")
        sys.stdout.flush()


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
    ap.add_argument("--cpu-window", action="store_true")
    ap.add_argument("--gpu-window", action="store_true")
    ap.add_argument("--sizes", nargs="*", default=["100x70"], help="--cpu-window: image sizes, W x H each")
    ap.add_argument("--window-leg", metavar="WORKLOAD")
    args = ap.parse_args()
    if args.window_leg:
        window_leg(args.window_leg)
    if args.cpu:
        cpu()
    if args.cpu_window:
        cpu_window([tuple(int(v) for v in s.split("x")) for s in args.sizes])
    if args.gpu_window:
        gpu_window(args.workloads, args.timeout)
    if args.gpu:
        gpu(args.parent_lib, args.workloads, args.timeout)
    if args.leg:
        leg(*args.leg)
    if not (args.cpu or args.gpu or args.leg or args.cpu_window or args.gpu_window or args.window_leg):
        print(__doc__)
