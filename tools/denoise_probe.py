#!/usr/bin/env python3
"""Measurements of the denoiser (rpt_denoise, csrc/k_denoise.h).

  python tools/denoise_probe.py --quality [out]     no GPU: the parameter grid against converged CPU-oracle images of DarkCornell (nee 0), VeachMIS (nee 1)
                                                    and PBRTest (nee 0) at 128 x 128 (8 spp noisy, 1024 spp converged); writes the table and the grid point with
                                                    the lowest summed error ratio — the defaults of rpt_denoise_params_default — to profiles/r11_denoise_quality.txt
  python tools/denoise_probe.py --quality-variance [out]   no GPU: the same oracle images and the moments record of the 8-spp image's samples; rpt_denoise_variance's grid
                                                    sigma_variance x iterations x sigma_color (the other parameters at rpt_denoise's defaults; sigma_variance = 0, the
                                                    plain filter, with every base setting) to profiles/r14_denoise_variance_quality.txt; its lowest summed ratio is
                                                    what rpt_denoise_var_params_default ships
  python tools/denoise_probe.py --gpu [out]         one MI355X: per workload (DarkCornell 1024^2, VeachMIS 1080p MIS, PBRTest 2048^2 textured) the 32-spp batch
                                                    time, guides_ms (median of 9 rebuilds), device_ms with cached guides (median of 25 calls after warm-up, device
                                                    events), the pass at step 1 and the pass at step 16 (5 passes - 4 passes), and rel-L2 of the noisy and the
                                                    denoised 32-spp image against a 4096-spp GPU render; writes profiles/r11_denoise.txt, above the record of the
                                                    wave-mapping comparison the file keeps.  (--workload NAME: one child run of it.)
  python tools/denoise_probe.py --gpu-variance [out]   one MI355X: per workload the 32-spp batch time (moments off, and on), device_ms of rpt_denoise and of
                                                    rpt_denoise_variance (own record on the device; the term off = the shipped default, and on at sigma_variance 4)
                                                    side by side, same base parameters, guides cached, device events, median of 25 calls; writes
                                                    profiles/r14_denoise_variance.txt, above the notes the file keeps at its foot
  python tools/denoise_probe.py --quality-temporal [out]   no GPU: a camera path of eight views per scene (100 x 70; 1, 2 and 4 spp per view, the accumulator zeroed at
                                                    every view as the reference does while the camera moves); rel-L2 of the LAST view against its 1024-spp oracle image
                                                    for the raw mean, rpt_denoise, rpt_denoise_variance (sigma_variance 8, three passes) and rpt_denoise_temporal over
                                                    the grid max_history x normal_min x plane_max x sigma_variance x iterations, the history chained through the eight
                                                    views by rpt_debug_denoise_temporal_host; writes profiles/r15_temporal_quality.txt; its lowest summed ratio is what
                                                    rpt_temporal_params_default ships
  python tools/denoise_probe.py --gpu-temporal [out]   one MI355X: per workload the 32-spp batch (moments on), then view A, then a moved view B: device_ms of
                                                    rpt_denoise_temporal with B's history reprojected beside rpt_denoise_variance with the same filter parameters,
                                                    guides cached, device events, median of 25 calls; writes profiles/r15_temporal.txt
  python tools/denoise_probe.py --quality-firefly [out]   no GPU: the firefly clamp (csrc/k_firefly.h) over clamp_scale {0, 1, 2, 4, 8} x clamp_radius {1, 2, 3}, clamp_floor 0, on
                                                    DarkCornell, VeachMIS (nee 1), PBRTest and DarkCornell with nee 1: rpt_denoise_variance at 8 spp (128 x 128; the shipped
                                                    filter defaults, and sigma_variance 8 with three passes) and the eight-view path of --quality-temporal at 1 / 2 / 4 spp
                                                    through rpt_denoise_temporal's shipped defaults; rel-L2 ratios against 1024-spp oracle images and the share of the
                                                    image's summed radiance the clamp removes; writes profiles/r16_firefly_quality.txt; the lowest summed ratio of the
                                                    first and of the third grid are the recommended settings hip.FIREFLY_CLAMP_VARIANCE / _TEMPORAL (the clamp ships off)
  python tools/denoise_probe.py --gpu-firefly [out]   one MI355X: per workload the 32-spp batch (moments on), then device_ms of rpt_denoise_variance and of
                                                    rpt_denoise_temporal (view B with A's history) with the clamp off and on (clamp_scale 2, clamp_radius 1 / 2 / 3),
                                                    guides cached, device events, median of 25 calls, and pixels_clamped; writes profiles/r16_firefly.txt.  Two more builds
                                                    of librpt_hip.so can be timed in the same run, each in processes of its own through RPT_HIP_LIB as tools/ab_libs.sh
                                                    does it: RPT_PARENT_LIB = the parent commit's (git worktree add DIR HEAD~1 && make -C DIR hip, then
                                                    DIR/rust-path-tracer_amd/lib/librpt_hip.so), whose clamp-off figures are taken between two runs of this build and
                                                    whose images are compared; RPT_VARIANT_LIB = a build of this commit with another clamp kernel (RPT_VARIANT_NAME
                                                    names it in the report), whose clamp-on figures are printed beside this build's
  python tools/denoise_probe.py --quality-glass [out]   no GPU: guides that follow glass (rpt_set_guides_through_glass, K = 2, 4, 8) against first-hit guides on the room and
                                                    the open scene of tests/model_scenes.py (128 x 128, 8 spp against 1024 spp of the restatement with models): rel-L2 over the
                                                    pixels whose chain crossed glass and over the whole image, rpt_denoise and rpt_denoise_variance at their shipped
                                                    defaults; writes profiles/r20_glass_guides_quality.txt; the K of the lowest summed error over the glass pixels is
                                                    hip.GUIDES_THROUGH_GLASS (the setting ships off)
"""
import hashlib
import importlib
import itertools
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

GRID = {"iterations": (1, 2, 3, 4, 5), "normal_power_log2": (0, 1, 3, 5, 7), "sigma_color": (0.0, 0.5, 0.75, 1.0, 1.5, 2.0, 4.0), "sigma_plane": (0.25, 0.5, 1.0, 2.0, 4.0), "demodulate": (0, 1)}
WORKLOADS = {"DarkCornell": ("DarkCornell", 1024, 1024, 0, False), "VeachMIS": ("VeachMIS", 1920, 1080, 1, False), "PBRTest": ("PBRTest", 2048, 2048, 0, True)}


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def quality(out_path):
    from oracle_ffi import Oracle
    import denoise_ref
    from denoise_ref import QUALITY, quality_images
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    orc = Oracle("rpt_math")
    worlds = {}
    world = lambda name: worlds.setdefault(name, rpt.World.from_path(rpt.fixture(name + ".glb")))
    sets = []
    for scene, nee in QUALITY:
        t0 = time.time()
        noisy, conv, g = quality_images(rpt, world, orc, scene, nee)
        sets.append((scene, nee, noisy, conv, g, rel_l2(noisy, conv)))
        print(f"{scene}: oracle images in {time.time() - t0:.0f} s, rel-L2 of the 8-spp mean {sets[-1][5]:.4f}", flush=True)
    rows = []
    keys = list(GRID)
    for values in itertools.product(*(GRID[k] for k in keys)):
        p = hip.denoise_params(**dict(zip(keys, values)))
        ratios = []
        for scene, nee, noisy, conv, g, e_noisy in sets:
            den = hip.denoise_host(noisy, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], p, 0)
            ratios.append(rel_l2(den, conv) / e_noisy)
        rows.append((sum(ratios), values, ratios))
    rows.sort(key=lambda r: r[0])
    d = hip.denoise_params()
    defaults = (d.iterations, d.normal_power_log2, d.sigma_color, d.sigma_plane, d.demodulate)
    lines = ["Denoiser quality against converged CPU-oracle images (tools/denoise_probe.py --quality): 128 x 128, the oracle's 8-spp mean denoised by",
             "rpt_debug_denoise_host over the numpy guides of tests/denoise_ref.py, rel-L2 against the oracle's 1024-spp mean; ratio = denoised / noisy (< 1: the filter helps).",
             "", "rel-L2 of the 8-spp mean: " + ", ".join(f"{s[0]} (nee {s[1]}) {s[5]:.4f}" for s in sets), ""]
    best = rows[0]
    lines.append(f"lowest summed ratio of the grid: {dict(zip(keys, best[1]))}  ->  " + ", ".join(f"{s[0]} {r:.3f}" for s, r in zip(sets, best[2])) + f"  (sum {best[0]:.3f})")
    mine = [r for r in rows if tuple(float(v) for v in r[1]) == tuple(float(v) for v in defaults)]
    lines.append(f"rpt_denoise_params_default: {dict(zip(keys, defaults))}  ->  " +
                 (", ".join(f"{s[0]} {r:.3f}" for s, r in zip(sets, mine[0][2])) + f"  (sum {mine[0][0]:.3f})" if mine else "not a grid point"))
    lines += ["", "grid (sorted by the summed ratio): " + " ".join(keys) + " | " + " ".join(s[0] for s in sets) + " | sum"]
    for total, values, ratios in rows:
        lines.append("  " + " ".join(f"{v:g}" for v in values) + " | " + " ".join(f"{r:.3f}" for r in ratios) + f" | {total:.3f}")
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines[:8]))


VAR_GRID = {"sigma_variance": (0.0, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0), "iterations": (1, 2, 3, 4, 5, 6), "sigma_color": (0.0, 0.5, 1.0, 2.0, 4.0)}


def quality_variance(out_path):
    from oracle_ffi import Oracle
    import denoise_var_ref
    from denoise_ref import QUALITY
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    orc = Oracle("rpt_math")
    worlds = {}
    world = lambda name: worlds.setdefault(name, rpt.World.from_path(rpt.fixture(name + ".glb")))
    sets = []
    for scene, nee in QUALITY:
        t0 = time.time()
        noisy, conv, g, moments, _ = denoise_var_ref.quality_inputs(rpt, world, orc, scene, nee)
        sets.append((scene, nee, noisy, conv, g, rel_l2(noisy, conv), moments))
        print(f"{scene}: oracle images in {time.time() - t0:.0f} s, rel-L2 of the 8-spp mean {sets[-1][5]:.4f}", flush=True)
    run = lambda p, s: hip.denoise_variance_host(s[2], s[4]["albedo"], s[4]["normal"], s[4]["position"], s[4]["depth"], s[4]["kind"], s[6], p, 0)[0]
    rows = []
    keys = list(VAR_GRID)
    for values in itertools.product(*(VAR_GRID[k] for k in keys)):
        p = hip.denoise_var_params(**dict(zip(keys, values)))
        ratios = [rel_l2(run(p, s), s[3]) / s[5] for s in sets]
        rows.append((sum(ratios), values, ratios))
    rows.sort(key=lambda r: r[0])
    show = lambda r: ", ".join(f"{s[0]} {x:.3f}" for s, x in zip(sets, r[2])) + f"  (sum {r[0]:.3f})"
    d, b = hip.denoise_var_params(), hip.denoise_params()
    shipped = (d.sigma_variance, d.base.iterations, d.base.sigma_color)
    plain = (0.0, b.iterations, b.sigma_color)
    find = lambda point: [r for r in rows if tuple(float(v) for v in r[1]) == tuple(float(v) for v in point)]
    measured = [int((s[6][..., 2] >= 2).sum()) for s in sets]
    zero = [int((denoise_var_ref.variance_of_mean(s[6]) == 0).sum()) for s in sets]
    lines = ["Variance-guided denoise (rpt_denoise_variance) against converged CPU-oracle images (tools/denoise_probe.py --quality-variance): the inputs of",
             "r11_denoise_quality.txt (128 x 128, the oracle's 8-spp mean, rel-L2 against its 1024-spp mean; ratio = denoised / noisy) and the moments record of the 8-spp",
             "image's samples (tests/denoise_var_ref.py quality_inputs), filtered by rpt_debug_denoise_variance_host over the numpy guides.  normal_power_log2 "
             f"{b.normal_power_log2}, sigma_plane {b.sigma_plane:g}, demodulate {b.demodulate}: rpt_denoise's defaults.", "",
             "rel-L2 of the 8-spp mean: " + ", ".join(f"{s[0]} (nee {s[1]}) {s[5]:.4f}" for s in sets),
             "pixels of 16384 with a zero empirical variance after 8 samples: " + ", ".join(f"{s[0]} {z}" for s, z in zip(sets, zero)) +
             "  (measured: " + ", ".join(str(m) for m in measured) + ")", "",
             f"lowest summed ratio of the grid: {dict(zip(keys, rows[0][1]))}  ->  " + show(rows[0])]
    for name, point in (("rpt_denoise_var_params_default", shipped), ("rpt_denoise's defaults (the plain filter: sigma_variance 0)", plain)):
        hit = find(point)
        lines.append(f"{name}: {dict(zip(keys, point))}  ->  " + (show(hit[0]) if hit else "not a grid point"))
    lines.append("best point per sigma_variance:")
    for sv in VAR_GRID["sigma_variance"]:
        r = [r for r in rows if r[1][0] == sv][0]
        lines.append(f"  sigma_variance {sv:g}: iterations {r[1][1]} sigma_color {r[1][2]:g}  ->  " + show(r))
    lines += ["", "grid (sorted by the summed ratio): " + " ".join(keys) + " | " + " ".join(s[0] for s in sets) + " | sum"]
    for total, values, ratios in rows:
        lines.append("  " + " ".join(f"{v:g}" for v in values) + " | " + " ".join(f"{r:.3f}" for r in ratios) + f" | {total:.3f}")
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines[:22]))


def gpu_child(workload):
    """one workload, in a process of its own; prints one JSON line"""
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    scene, W, H, nee, textured = WORKLOADS[workload]
    if textured:
        from scenes import pbrtest_textured_scene
        made = pbrtest_textured_scene()
        world = made[0] if isinstance(made, tuple) else made
    else:
        world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
    r = hip.Renderer(0)
    r.upload_scene(world)
    cfg = rpt.default_config(W, H, nee=nee)
    r.set_config(cfg)
    seeds = rpt.blue_noise_seeds(W, H)
    out = {"workload": workload, "width": W, "height": H}
    r.reset(seeds)
    r.render(32)                                         # warm-up batch (allocations, clocks)
    batch = []
    for _ in range(5):
        r.reset(seeds)
        t0 = time.perf_counter()
        r.render(32)
        batch.append((time.perf_counter() - t0) * 1e3)
    out["batch_ms"] = float(np.median(batch))
    noisy = r.resolve(0)
    den, rep = r.denoise(with_report=True)
    out["guides_ms_first_use"], rebuilds = rep["guides_ms"], []           # the first use allocates the buffers too
    for _ in range(9):
        r.set_config(cfg)                                # marks the guides stale; the accumulator stays
        rep = r.denoise(with_report=True)[1]
        assert rep["guides_rebuilt"] == 1
        rebuilds.append(rep["guides_ms"])
    out["guides_ms"], out["guides_ms_min_max"] = float(np.median(rebuilds)), [float(min(rebuilds)), float(max(rebuilds))]
    d = hip.denoise_params()
    out["defaults"] = {"iterations": d.iterations, "normal_power_log2": d.normal_power_log2, "sigma_color": d.sigma_color, "sigma_plane": d.sigma_plane, "demodulate": d.demodulate}
    for _ in range(3):
        r.denoise()
    ms = [r.denoise(with_report=True)[1]["device_ms"] for _ in range(25)]
    out["device_ms"] = float(np.median(ms))
    out["device_ms_min_max"] = [float(min(ms)), float(max(ms))]
    per_pass, digest = {}, hashlib.sha256(den.tobytes())
    for it in (1, 4, 5):                                 # 1 pass = step 1 only; the fifth pass is the one at step 16
        p = hip.denoise_params(iterations=it)
        digest.update(r.denoise(params=p).tobytes())
        per_pass[it] = float(np.median([r.denoise(params=p, with_report=True)[1]["device_ms"] for _ in range(25)]))
    out["device_ms_1_pass_step_1"] = per_pass[1]
    out["device_ms_4_passes"], out["device_ms_5_passes"] = per_pass[4], per_pass[5]
    out["device_ms_pass_at_step_16"] = per_pass[5] - per_pass[4]
    out["output_sha256"] = digest.hexdigest()[:16]       # of the 2-, 1-, 4- and 5-pass images: two builds that filter alike print the same
    for _ in range(127):                                 # 32 + 127 x 32 = 4096 spp: the same accumulator, continued
        r.render(32)
    ref = r.resolve(0)
    ok = np.isfinite(ref).all(axis=-1) & np.isfinite(noisy).all(axis=-1) & np.isfinite(den).all(axis=-1)
    out["pixels_compared"] = int(ok.sum())
    out["rel_l2_noisy"], out["rel_l2_denoised"] = rel_l2(noisy[ok], ref[ok]), rel_l2(den[ok], ref[ok])
    r.close()
    print("RESULT " + json.dumps(out), flush=True)


def gpu_variance_child(workload):
    """rpt_denoise and rpt_denoise_variance side by side on one workload, in a process of its own; prints one JSON line"""
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    scene, W, H, nee, textured = WORKLOADS[workload]
    if textured:
        from scenes import pbrtest_textured_scene
        made = pbrtest_textured_scene()
        world = made[0] if isinstance(made, tuple) else made
    else:
        world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
    r = hip.Renderer(0)
    r.upload_scene(world)
    r.set_config(rpt.default_config(W, H, nee=nee))
    seeds = rpt.blue_noise_seeds(W, H)
    out = {"workload": workload, "width": W, "height": H}

    def batch():
        times = []
        for _ in range(6):                               # the first is the warm-up (allocations, clocks)
            r.reset(seeds)
            t0 = time.perf_counter()
            r.render(32)
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times[1:]))
    out["batch_ms"] = batch()
    r.set_moments(True)
    out["batch_ms_moments"] = batch()                    # leaves 32 spp and their moments
    median = lambda call: float(np.median([call()[-1]["device_ms"] for _ in range(28)][3:]))
    d = hip.denoise_var_params()
    out["defaults"] = {"sigma_variance": d.sigma_variance, "iterations": d.base.iterations, "sigma_color": d.base.sigma_color}
    digest = hashlib.sha256()
    for it in (d.base.iterations, 1, 5):
        plain, off, on = hip.denoise_params(iterations=it), hip.denoise_var_params(iterations=it, sigma_variance=0.0), hip.denoise_var_params(iterations=it, sigma_variance=4.0)
        a, b, c = r.denoise(params=plain), r.denoise_variance(params=off)[0], r.denoise_variance(params=on)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))              # the term off: rpt_denoise's bytes
        digest.update(c[0].tobytes() + c[1].tobytes())
        out[f"plain_ms_{it}"] = median(lambda: r.denoise(params=plain, with_report=True))
        out[f"var_off_ms_{it}"] = median(lambda: r.denoise_variance(params=off, with_report=True))
        out[f"var_on_ms_{it}"] = median(lambda: r.denoise_variance(params=on, with_report=True))
    out["iterations"] = d.base.iterations
    out["output_sha256"] = digest.hexdigest()[:16]
    r.close()
    print("RESULT " + json.dumps(out), flush=True)


FOOT_RECORD = "notes kept by hand"


def gpu_variance(out_path):
    results = []
    for workload in WORKLOADS:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload-variance", workload], capture_output=True, text=True, timeout=300)
        line = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
        if run.returncode != 0 or not line:
            print(run.stdout[-2000:], run.stderr[-2000:])
            raise SystemExit(f"{workload} failed with status {run.returncode}: nothing more is started on the GPU")
        results.append(json.loads(line[0][7:]))
        print(line[0], flush=True)
    n = results[0]["iterations"]
    lines = ["rpt_denoise_variance beside rpt_denoise on one MI355X (tools/denoise_probe.py --gpu-variance): 32-spp batches; the same base parameters for both calls",
             f"(rpt_denoise's defaults but for the number of passes); rpt_denoise_variance reads the context's own moments record on the device.  shipped defaults {json.dumps(results[0]['defaults'])}.",
             "device_ms: HIP events around pre-pass + passes, guides cached, median of 25 calls after 3 warm-up calls; batch: host clock around rpt_render(32), median of 5 after a warm-up.",
             "term off: sigma_variance 0 (k_dn_pass_var without the 3 x 3 variance reads; the image is rpt_denoise's, checked bitwise in this run); term on: sigma_variance 4.", ""]
    worst = 0.0
    for res in results:
        lines.append(f"{res['workload']} {res['width']}x{res['height']}: batch {res['batch_ms']:.2f} ms (moments on {res['batch_ms_moments']:.2f} ms); output sha256 {res['output_sha256']}")
        for it in (n, 1, 5):
            p, off, on = res[f"plain_ms_{it}"], res[f"var_off_ms_{it}"], res[f"var_on_ms_{it}"]
            lines.append(f"    {it} pass{'es' if it > 1 else '  '}: rpt_denoise {p:.3f} ms | rpt_denoise_variance term off {off:.3f} ms ({off / p:.2f} x), term on {on:.3f} ms ({on / p:.2f} x) = "
                         f"{100 * on / res['batch_ms']:.1f} % of the batch")
        worst = max(worst, res[f"var_on_ms_{n}"] / res["batch_ms"], res[f"var_off_ms_{n}"] / res["batch_ms"])
    lines += ["", f"condition (rpt_denoise_variance at the shipped number of passes, guides cached, < the 32-spp batch it follows): worst share {100 * worst:.1f} % -> {'HELD' if worst < 1 else 'MISSED'}"]
    if os.path.exists(out_path):
        old = open(out_path).read().splitlines()
        at = [k for k, l in enumerate(old) if l.startswith(FOOT_RECORD)]
        if at:
            lines += [""] + old[at[0]:]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


TEMPORAL_GRID = {"max_history": (8.0, 32.0, 128.0, float("inf")), "normal_min": (0.5, 0.9, 0.99), "plane_max": (0.5, 2.0, 8.0), "sigma_variance": (0.0, 2.0, 8.0, 32.0),
                 "iterations": (2, 3)}
PATH_VIEWS, PATH_SPP, PATH_SIZE = 8, (1, 2, 4), (100, 70)


def path_camera(cfg, k):
    """view k of the path: the default camera dragged sideways and yawed, a steady 0.05 units and 0.02 rad per view"""
    c = cfg.copy()
    c.cam_position[0] += 0.05 * k
    c.cam_rotation[1] += 0.02 * k
    return c


def quality_temporal(out_path):
    from oracle_ffi import Oracle
    import denoise_ref
    import denoise_var_ref
    from denoise_ref import QUALITY
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    orc = Oracle("rpt_math")
    F = np.float32
    W, H = PATH_SIZE
    paths = []                                           # (scene, nee, spp, [(cfg, mean, guides, moments)] per view, converged mean of the last view)
    for scene, nee in QUALITY:
        t0 = time.time()
        w = rpt.World.from_path(rpt.fixture(scene + ".glb"))
        sc = orc.scene(w)
        cfgs = [path_camera(rpt.default_config(W, H, nee=nee), k) for k in range(PATH_VIEWS)]
        guides = [denoise_ref.guides(w, c, orc, sc) for c in cfgs]
        for spp in PATH_SPP:
            rng = rpt.blue_noise_seeds(W, H)
            views = []
            for c, g in zip(cfgs, guides):               # every view from a zero accumulator, the rng carried on
                moments, acc = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
                for _ in range(spp):
                    smp, rng, _ = orc.trace_cpu(c, sc, rng, 1)
                    denoise_var_ref.moments_add(moments, smp[..., :3])
                    acc = (acc + smp).astype(F)
                views.append((c, (acc[..., :3] / F(spp)).astype(F), g, moments))
            conv, _, _ = orc.trace_cpu(cfgs[-1], sc, rng, 1024)
            paths.append((scene, nee, spp, views, (conv[..., :3] / F(1024)).astype(F)))
        print(f"{scene}: oracle images in {time.time() - t0:.0f} s", flush=True)

    def temporal(path, p):
        prev = None
        for c, mean, g, moments in path[3]:
            out = hip.denoise_temporal_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], moments, c, prev, p, 0)
            prev = {"camera": c, "normal": g["normal"], "position": g["position"], "kind": g["kind"], "records": out["records"]}
        return out

    raw = [rel_l2(path[3][-1][1], path[4]) for path in paths]
    last = lambda path: (path[3][-1][1],) + tuple(path[3][-1][2][k] for k in ("albedo", "normal", "position", "depth", "kind"))
    plain = [rel_l2(hip.denoise_host(*last(path), None, 0), path[4]) / e for path, e in zip(paths, raw)]
    vp = hip.denoise_var_params(sigma_variance=8.0, iterations=3)
    var = [rel_l2(hip.denoise_variance_host(*last(path), path[3][-1][3], vp, 0)[0], path[4]) / e for path, e in zip(paths, raw)]
    keys = list(TEMPORAL_GRID)
    rows = []
    t0 = time.time()
    for values in itertools.product(*(TEMPORAL_GRID[k] for k in keys)):
        p = hip.temporal_params(**dict(zip(keys, values)))
        ratios = [rel_l2(temporal(path, p)["rgb"], path[4]) / e for path, e in zip(paths, raw)]
        rows.append((sum(ratios), values, ratios))
    rows.sort(key=lambda r: r[0])
    print(f"grid of {len(rows)} points in {time.time() - t0:.0f} s", flush=True)
    names = [f"{path[0]}@{path[2]}" for path in paths]
    show = lambda ratios: " ".join(f"{r:.3f}" for r in ratios) + f" | {sum(ratios):.3f}"
    d = hip.temporal_params()
    shipped = (d.max_history, d.normal_min, d.plane_max, d.filter.sigma_variance, d.filter.base.iterations)
    hit = [r for r in rows if tuple(float(v) for v in r[1]) == tuple(float(v) for v in shipped)]
    with_history = [temporal(path, hip.temporal_params(**dict(zip(keys, rows[0][1]))))["pixels_with_history"] for path in paths]
    b = hip.denoise_params()
    lines = ["Temporal reuse (rpt_denoise_temporal) against converged CPU-oracle images (tools/denoise_probe.py --quality-temporal): a camera path of "
             f"{PATH_VIEWS} views per scene at {W} x {H},",
             "0.05 units sideways and 0.02 rad of yaw per view, the accumulator zeroed at every view, the rng carried on; 1, 2 and 4 spp per view (SCENE@spp below).",
             "rel-L2 of the LAST view against a 1024-spp oracle image of that view; ratio = filtered / raw (< 1: the filter helps).  The history is chained through the",
             "eight views by rpt_debug_denoise_temporal_host over the numpy guides of tests/denoise_ref.py.  The base parameters that are not in the grid are rpt_denoise's",
             f"defaults (normal_power_log2 {b.normal_power_log2}, sigma_color {b.sigma_color:g}, sigma_plane {b.sigma_plane:g}, demodulate {b.demodulate}).", "",
             "columns: " + " ".join(names) + " | sum",
             "rel-L2 of the raw mean:                          " + " ".join(f"{e:.4f}" for e in raw),
             "rpt_denoise, defaults:                           " + show(plain),
             "rpt_denoise_variance, sigma_variance 8, 3 passes: " + show(var),
             f"rpt_denoise_temporal, lowest summed ratio {dict(zip(keys, rows[0][1]))}: " + show(rows[0][2]),
             f"    pixels of {W * H} with history in the last view at that point: " + " ".join(str(n) for n in with_history),
             f"rpt_temporal_params_default {dict(zip(keys, shipped))}: " + (show(hit[0][2]) if hit else "not a grid point"),
             "best point per sigma_variance:"]
    for sv in TEMPORAL_GRID["sigma_variance"]:
        r = [r for r in rows if r[1][3] == sv][0]
        lines.append(f"  sigma_variance {sv:g}: {dict(zip(keys, r[1]))}  ->  " + show(r[2]))
    lines += ["", "grid (sorted by the summed ratio): " + " ".join(keys) + " | " + " ".join(names) + " | sum"]
    for total, values, ratios in rows:
        lines.append("  " + " ".join(f"{v:g}" for v in values) + " | " + show(ratios))
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines[:20]))


def gpu_temporal_child(workload):
    """rpt_denoise_temporal beside rpt_denoise_variance on one workload, in a process of its own; prints one JSON line"""
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    scene, W, H, nee, textured = WORKLOADS[workload]
    if textured:
        from scenes import pbrtest_textured_scene
        made = pbrtest_textured_scene()
        world = made[0] if isinstance(made, tuple) else made
    else:
        world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
    r = hip.Renderer(0)
    r.upload_scene(world)
    cfg_a = rpt.default_config(W, H, nee=nee)
    cfg_b = path_camera(cfg_a, 4)
    r.set_config(cfg_a)
    r.set_moments(True)
    seeds = rpt.blue_noise_seeds(W, H)
    out = {"workload": workload, "width": W, "height": H}
    times = []
    for _ in range(6):                                   # the first is the warm-up (allocations, clocks); leaves 32 spp of view A and their moments
        r.reset(seeds)
        t0 = time.perf_counter()
        r.render(32)
        times.append((time.perf_counter() - t0) * 1e3)
    out["batch_ms"] = float(np.median(times[1:]))
    d = hip.temporal_params()
    out["defaults"] = {"max_history": d.max_history, "normal_min": d.normal_min, "plane_max": d.plane_max, "sigma_variance": d.filter.sigma_variance, "iterations": d.filter.base.iterations}
    on = hip.temporal_params(sigma_variance=4.0)
    first = r.denoise_temporal(params=d, with_report=True)
    assert first[3]["pixels_with_history"] == 0
    plain = r.denoise_variance(params=d.filter)
    assert np.array_equal(first[0].view(np.uint32), plain[0].view(np.uint32))     # no history: rpt_denoise_variance's bytes
    r.set_config(cfg_b)
    r.reset(seeds)
    r.render(32)
    median = lambda call: float(np.median([call()[-1]["device_ms"] for _ in range(28)][3:]))
    digest = hashlib.sha256()
    for name, p in (("default", d), ("on", on)):
        got = r.denoise_temporal(params=p, with_report=True)         # every call of this epoch blends with view A's history
        assert got[3]["history_state"] == 1
        out[f"with_history_{name}"] = got[3]["pixels_with_history"]
        digest.update(got[0].tobytes() + got[1].tobytes() + got[2].tobytes())
        out[f"temporal_ms_{name}"] = median(lambda: r.denoise_temporal(params=p, with_report=True))
        out[f"variance_ms_{name}"] = median(lambda: r.denoise_variance(params=p.filter, with_report=True))
    out["output_sha256"] = digest.hexdigest()[:16]
    r.close()
    print("RESULT " + json.dumps(out), flush=True)


def gpu_temporal(out_path):
    results = []
    for workload in WORKLOADS:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload-temporal", workload], capture_output=True, text=True, timeout=300)
        line = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
        if run.returncode != 0 or not line:
            print(run.stdout[-2000:], run.stderr[-2000:])
            raise SystemExit(f"{workload} failed with status {run.returncode}: nothing more is started on the GPU")
        results.append(json.loads(line[0][7:]))
        print(line[0], flush=True)
    lines = ["rpt_denoise_temporal beside rpt_denoise_variance on one MI355X (tools/denoise_probe.py --gpu-temporal): 32-spp batches with moments on; view A, then view B",
             "(0.2 units sideways, 0.08 rad of yaw), whose calls reproject A's history; both calls with the same filter parameters and the context's own moments record.",
             f"shipped defaults {json.dumps(results[0]['defaults'])}; 'term on': the same with sigma_variance 4.",
             "device_ms: HIP events around the fused temporal kernel (or the pre-pass), the two guide copies and the passes, guides cached, median of 25 calls after 3 warm-up",
             "calls; batch: host clock around rpt_render(32), median of 5 after a warm-up.", ""]
    worst = 0.0
    for res in results:
        lines.append(f"{res['workload']} {res['width']}x{res['height']}: batch {res['batch_ms']:.2f} ms; output sha256 {res['output_sha256']}")
        for name, label in (("default", "defaults"), ("on", "term on ")):
            t, v = res[f"temporal_ms_{name}"], res[f"variance_ms_{name}"]
            lines.append(f"    {label}: rpt_denoise_variance {v:.3f} ms | rpt_denoise_temporal {t:.3f} ms ({t / v:.2f} x) = {100 * t / res['batch_ms']:.1f} % of the batch; "
                         f"{res[f'with_history_{name}']} of {res['width'] * res['height']} pixels with history")
            worst = max(worst, t / res["batch_ms"])
    lines += ["", f"condition (rpt_denoise_temporal, guides cached, < the 32-spp batch it follows): worst share {100 * worst:.1f} % -> {'HELD' if worst < 1 else 'MISSED'}"]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


MAPPING_RECORD = "wave mapping of a pass"


def gpu(out_path):
    results = []
    for workload in WORKLOADS:
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload", workload], capture_output=True, text=True, timeout=420)
        line = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
        if run.returncode != 0 or not line:
            print(run.stdout[-2000:], run.stderr[-2000:])
            raise SystemExit(f"{workload} failed with status {run.returncode}: nothing more is started on the GPU")
        results.append(json.loads(line[0][7:]))
        print(line[0], flush=True)
    lines = ["rpt_denoise on one MI355X (tools/denoise_probe.py --gpu): 32-spp batches, default parameters " + json.dumps(results[0]["defaults"]) + ".",
             "device_ms: HIP events around pre-pass + passes, guides cached, median of 25 calls after 4 warm-up calls; batch_ms: host clock around rpt_render(32), median of 5;",
             "guides: median of 9 rebuilds after rpt_set_config (the first use, which also allocates, apart); pass at step 16 = 5 passes - 4 passes.", ""]
    for res in results:
        lines.append(f"{res['workload']} {res['width']}x{res['height']}: batch {res['batch_ms']:.2f} ms, guides {res['guides_ms']:.3f} ms (min {res['guides_ms_min_max'][0]:.3f}, "
                     f"max {res['guides_ms_min_max'][1]:.3f}; first use {res['guides_ms_first_use']:.3f}), "
                     f"denoise {res['device_ms']:.3f} ms (min {res['device_ms_min_max'][0]:.3f}, max {res['device_ms_min_max'][1]:.3f}) = {100 * res['device_ms'] / res['batch_ms']:.1f} % of the batch; "
                     f"pass at step 1 {res['device_ms_1_pass_step_1']:.3f} ms, pass at step 16 {res['device_ms_pass_at_step_16']:.3f} ms (4 passes {res['device_ms_4_passes']:.3f}, "
                     f"5 passes {res['device_ms_5_passes']:.3f}); rel-L2 vs 4096 spp: noisy {res['rel_l2_noisy']:.4f}, denoised {res['rel_l2_denoised']:.4f}; output sha256 {res['output_sha256']}")
    worst = max(res["device_ms"] / res["batch_ms"] for res in results)
    lines += ["", f"condition (device_ms with cached guides < the 32-spp batch it follows): worst share {100 * worst:.1f} % -> {'HELD' if worst < 1 else 'MISSED'}"]
    if os.path.exists(out_path):                         # the mapping comparison was taken once, with a build that had both kernels: kept as it is
        old = open(out_path).read().splitlines()
        at = [k for k, l in enumerate(old) if l.startswith(MAPPING_RECORD)]
        if at:
            lines += [""] + old[at[0]:]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


FIREFLY_GRID = {"clamp_scale": (0.0, 1.0, 2.0, 4.0, 8.0), "clamp_radius": (1, 2, 3)}
FIREFLY_SCENES = [("DarkCornell", 0), ("VeachMIS", 1), ("PBRTest", 0), ("DarkCornell", 1)]


def quality_firefly(out_path):
    from oracle_ffi import Oracle
    import denoise_ref
    import denoise_var_ref
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    orc = Oracle("rpt_math")
    F = np.float32
    worlds = {}
    world = lambda name: worlds.setdefault(name, rpt.World.from_path(rpt.fixture(name + ".glb")))
    keys = list(FIREFLY_GRID)
    points = list(itertools.product(*(FIREFLY_GRID[k] for k in keys)))
    planes = lambda g: tuple(g[k] for k in ("albedo", "normal", "position", "depth", "kind"))

    def lost(mean, g, moments, point, demodulated):
        """the share of the image's summed radiance the clamp removes, and the clamped pixels"""
        if point[0] == 0.0:
            return 0.0, 0
        c, _, mask = hip.firefly_host(mean, g["albedo"], g["kind"], moments, counts=moments[..., 2], clamp_scale=point[0], clamp_floor=0.0, clamp_radius=point[1], demodulated=demodulated)
        return float(1.0 - c.astype(np.float64).sum() / mean.astype(np.float64).sum()), int(mask.sum())

    # -- rpt_denoise_variance at 8 spp
    sets = []
    for scene, nee in FIREFLY_SCENES:
        t0 = time.time()
        noisy, conv, g, moments, _ = denoise_var_ref.quality_inputs(rpt, world, orc, scene, nee)
        sets.append((f"{scene}/nee{nee}", noisy, conv, g, moments, rel_l2(noisy, conv)))
        print(f"{scene} nee {nee}: oracle images in {time.time() - t0:.0f} s, rel-L2 of the 8-spp mean {sets[-1][5]:.4f}", flush=True)
    d = hip.denoise_var_params()
    filters = [("the shipped filter defaults", dict(sigma_variance=d.sigma_variance, iterations=d.base.iterations)),
               ("the setting for scenes with NEE: sigma_variance 8, three passes", dict(sigma_variance=8.0, iterations=3))]
    var_tables = []
    for _, f in filters:
        rows = []
        for point in points:
            p = hip.denoise_var_params(clamp_scale=point[0], clamp_floor=0.0, clamp_radius=point[1], **f)
            dem = p.base.iterations != 0 and p.base.demodulate != 0
            ratios = [rel_l2(hip.denoise_variance_host(s[1], *planes(s[3]), s[4], p, 0)[0], s[2]) / s[5] for s in sets]
            gone = [lost(s[1], s[3], s[4], point, dem) for s in sets]
            rows.append((sum(ratios), point, ratios, gone))
        rows.sort(key=lambda r: (r[0], r[1]))
        var_tables.append(rows)
    print("variance grids done", flush=True)

    # -- the eight-view path through rpt_denoise_temporal
    W, H = PATH_SIZE
    paths = []
    for scene, nee in FIREFLY_SCENES:
        t0 = time.time()
        w = world(scene)
        sc = orc.scene(w)
        cfgs = [path_camera(rpt.default_config(W, H, nee=nee), k) for k in range(PATH_VIEWS)]
        guides = [denoise_ref.guides(w, c, orc, sc) for c in cfgs]
        for spp in PATH_SPP:
            rng = rpt.blue_noise_seeds(W, H)
            views = []
            for c, g in zip(cfgs, guides):               # every view from a zero accumulator, the rng carried on (as --quality-temporal)
                moments, acc = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
                for _ in range(spp):
                    smp, rng, _ = orc.trace_cpu(c, sc, rng, 1)
                    denoise_var_ref.moments_add(moments, smp[..., :3])
                    acc = (acc + smp).astype(F)
                views.append((c, (acc[..., :3] / F(spp)).astype(F), g, moments))
            conv, _, _ = orc.trace_cpu(cfgs[-1], sc, rng, 1024)
            paths.append((f"{scene}/nee{nee}@{spp}", views, (conv[..., :3] / F(1024)).astype(F)))
        print(f"{scene} nee {nee}: path images in {time.time() - t0:.0f} s", flush=True)

    def temporal(path, p):
        prev = None
        for c, mean, g, moments in path[1]:
            out = hip.denoise_temporal_host(mean, *planes(g), moments, c, prev, p, 0)
            prev = {"camera": c, "normal": g["normal"], "position": g["position"], "kind": g["kind"], "records": out["records"]}
        return out

    raw = [rel_l2(path[1][-1][1], path[2]) for path in paths]
    tp_rows = []
    for point in points:
        p = hip.temporal_params(clamp_scale=point[0], clamp_floor=0.0, clamp_radius=point[1])
        dem = p.filter.base.iterations != 0 and p.filter.base.demodulate != 0
        ratios = [rel_l2(temporal(path, p)["rgb"], path[2]) / e for path, e in zip(paths, raw)]
        gone = [lost(path[1][-1][1], path[1][-1][2], path[1][-1][3], point, dem) for path in paths]
        tp_rows.append((sum(ratios), point, ratios, gone))
    tp_rows.sort(key=lambda r: (r[0], r[1]))

    show = lambda r: " ".join(f"{x:.3f}" for x in r[2]) + f" | {r[0]:.3f} | " + " ".join(f"{100 * g[0]:.1f}%/{g[1]}" for g in r[3])
    fmt = lambda point: " ".join(f"{v:g}" for v in point)
    t = hip.temporal_params()
    lines = ["The firefly clamp (csrc/k_firefly.h; clamp_scale, clamp_floor, clamp_radius of rpt_denoise_var_params) against converged CPU-oracle images",
             "(tools/denoise_probe.py --quality-firefly): rel-L2 of the filtered image against the oracle's 1024-spp mean, ratio = filtered / raw mean (< 1: the call helps),",
             "through the host hooks over the numpy guides of tests/denoise_ref.py.  clamp_floor 0 throughout.  clamp_scale 0 = the clamp off (the radius is then not read:",
             "its three rows are one point).  After the sum: the share of the image's summed radiance that the clamp removes from the raw mean (of the last view, for a path)",
             "and the number of clamped pixels — the clamp is biased, and this is the bias.", ""]
    names = [s[0] for s in sets]
    for (title, f), rows in zip(filters, var_tables):
        lines += [f"== rpt_denoise_variance, 8 spp, 128 x 128, {title} ({json.dumps(f)})",
                  "rel-L2 of the 8-spp mean: " + ", ".join(f"{s[0]} {s[5]:.4f}" for s in sets),
                  f"lowest summed ratio: {dict(zip(keys, rows[0][1]))}",
                  "grid (sorted by the summed ratio): " + " ".join(keys) + " | " + " ".join(names) + " | sum | lost/pixels per scene"]
        lines += ["  " + fmt(r[1]) + " | " + show(r) for r in rows] + [""]
    lines += [f"== rpt_denoise_temporal, the eight-view path of --quality-temporal ({W} x {H}, SCENE@spp), rpt_temporal_params_default's other fields "
              f"(max_history {t.max_history:g}, normal_min {t.normal_min:g}, plane_max {t.plane_max:g}, sigma_variance {t.filter.sigma_variance:g}, iterations {t.filter.base.iterations})",
              "rel-L2 of the raw mean of the last view: " + ", ".join(f"{path[0]} {e:.4f}" for path, e in zip(paths, raw)),
              f"lowest summed ratio: {dict(zip(keys, tp_rows[0][1]))}",
              "grid (sorted by the summed ratio): " + " ".join(keys) + " | " + " ".join(path[0] for path in paths) + " | sum | lost/pixels per path"]
    lines += ["  " + fmt(r[1]) + " | " + show(r) for r in tp_rows] + [""]
    shipped_v, shipped_t = (d.clamp_scale, d.clamp_radius), (t.filter.clamp_scale, t.filter.clamp_radius)
    lines += ["The clamp ships OFF in both sets of defaults (a call that does not ask for it returns what it returned before the fields existed); the minima above are the",
              "recommended settings (hip.FIREFLY_CLAMP_VARIANCE, hip.FIREFLY_CLAMP_TEMPORAL), and the defaults carry their clamp_radius:",
              f"rpt_denoise_var_params_default ships clamp_scale {shipped_v[0]:g} clamp_radius {shipped_v[1]}; the first grid's minimum is {fmt(var_tables[0][0][1])}",
              f"rpt_temporal_params_default ships clamp_scale {shipped_t[0]:g} clamp_radius {shipped_t[1]}; the third grid's minimum is {fmt(tp_rows[0][1])}",
              f"for scenes with NEE (second grid) the minimum is {fmt(var_tables[1][0][1])}"]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def gpu_firefly_child(workload):
    """rpt_denoise_variance and rpt_denoise_temporal with the clamp off and on, on one workload, in a process of its own; prints one JSON line.  With
    RPT_PROBE_OFF_ONLY set (RPT_HIP_LIB names a build from before the clamp, which does not read the words) only the clamp-off figures are taken."""
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    scene, W, H, nee, textured = WORKLOADS[workload]
    if textured:
        from scenes import pbrtest_textured_scene
        made = pbrtest_textured_scene()
        world = made[0] if isinstance(made, tuple) else made
    else:
        world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
    other = bool(os.environ.get("RPT_PROBE_OFF_ONLY"))
    r = hip.Renderer(0)
    r.upload_scene(world)
    cfg_a = rpt.default_config(W, H, nee=nee)
    cfg_b = path_camera(cfg_a, 4)
    r.set_config(cfg_a)
    r.set_moments(True)
    seeds = rpt.blue_noise_seeds(W, H)
    out = {"workload": workload, "width": W, "height": H, "lib": os.environ.get("RPT_HIP_LIB", "")}
    times = []
    for _ in range(6):                                   # the first is the warm-up (allocations, clocks); leaves 32 spp of view A and their moments
        r.reset(seeds)
        t0 = time.perf_counter()
        r.render(32)
        times.append((time.perf_counter() - t0) * 1e3)
    out["batch_ms"] = float(np.median(times[1:]))

    def median(call):
        ms = [call()[-1]["device_ms"] for _ in range(28)][3:]
        return [float(np.median(ms)), float(min(ms)), float(max(ms))]
    settings = [("off", {})] + ([] if other else [(f"r{k}", dict(clamp_scale=2.0, clamp_radius=k)) for k in (1, 2, 3)])
    d = hip.temporal_params()
    r.denoise_temporal(params=d)                         # view A's history
    r.set_config(cfg_b)
    r.reset(seeds)
    r.render(32)
    digest = hashlib.sha256()
    for name, fields in settings:
        vp, tp = hip.denoise_var_params(**fields), hip.temporal_params(**fields)
        v, t = r.denoise_variance(params=vp, with_report=True), r.denoise_temporal(params=tp, with_report=True)
        assert t[3]["history_state"] == 1
        if name == "off":
            digest.update(v[0].tobytes() + v[1].tobytes() + t[0].tobytes() + t[1].tobytes() + t[2].tobytes())
        if not other:
            out[f"clamped_{name}"] = [v[2]["pixels_clamped"], t[3]["pixels_clamped"]]
        out[f"variance_ms_{name}"] = median(lambda: r.denoise_variance(params=vp, with_report=True))
        out[f"temporal_ms_{name}"] = median(lambda: r.denoise_temporal(params=tp, with_report=True))
    out["off_sha256"] = digest.hexdigest()[:16]           # of the clamp-off images: two builds that filter alike print the same
    r.close()
    print("RESULT " + json.dumps(out), flush=True)


VARIANT_NAME = os.environ.get("RPT_VARIANT_NAME", "RPT_VARIANT_LIB")


def gpu_firefly(out_path, parent_lib, variant_lib):
    def child(workload, lib, off_only=False):
        env = dict(os.environ)
        env.pop("RPT_HIP_LIB", None)
        env.pop("RPT_PROBE_OFF_ONLY", None)
        if lib:
            env["RPT_HIP_LIB"] = lib
        if off_only:
            env["RPT_PROBE_OFF_ONLY"] = "1"
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--workload-firefly", workload], capture_output=True, text=True, timeout=300, env=env)
        line = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
        if run.returncode != 0 or not line:
            print(run.stdout[-2000:], run.stderr[-2000:])
            raise SystemExit(f"{workload} failed with status {run.returncode}: nothing more is started on the GPU")
        print(line[0], flush=True)
        return json.loads(line[0][7:])
    f3 = lambda m: f"{m[0]:.3f} ms (min {m[1]:.3f}, max {m[2]:.3f})"
    lines = ["The firefly clamp on one MI355X (tools/denoise_probe.py --gpu-firefly): 32-spp batches with moments on; view A, then view B (0.2 units sideways, 0.08 rad of yaw),",
             "whose rpt_denoise_temporal calls reproject A's history.  The shipped defaults of both calls but for the clamp: off, and clamp_scale 2 at clamp_radius 1 / 2 / 3",
             "(k_dn_prepare_var_clamp / k_dn_temporal_clamp in place of k_dn_prepare_var / k_dn_temporal; each workgroup stages the (b, kind) of its 64 x 4 pixels and their halo in LDS).",
             "device_ms: HIP events around pre-pass (or the fused temporal kernel and the two guide copies) + passes, guides cached, median (min, max) of 25 calls after 3 warm-up",
             "calls; batch: host clock around rpt_render(32), median of 5 after a warm-up; pixels clamped: rpt_denoise_report.pixels_clamped.", ""]
    worst, inside = 0.0, True
    for workload in WORKLOADS:
        first = child(workload, None)
        parent = child(workload, parent_lib, True) if parent_lib else None
        variant = child(workload, variant_lib) if variant_lib else None
        second = child(workload, None) if parent_lib else None
        n = first["width"] * first["height"]
        lines.append(f"{workload} {first['width']}x{first['height']}: batch {first['batch_ms']:.2f} ms")
        for call in ("variance", "temporal"):
            off = first[f"{call}_ms_off"]
            lines.append(f"    rpt_denoise_{call}, clamp off: {f3(off)} = {100 * off[0] / first['batch_ms']:.1f} % of the batch")
            for k in (1, 2, 3):
                on = first[f"{call}_ms_r{k}"]
                lines.append(f"        clamp_scale 2 radius {k}: {f3(on)} ({on[0] / off[0]:.2f} x, +{on[0] - off[0]:.3f} ms) = {100 * on[0] / first['batch_ms']:.1f} % of the batch; "
                             f"{first[f'clamped_r{k}'][call == 'temporal']} of {n} pixels clamped")
                worst = max(worst, on[0] / first["batch_ms"])
                if variant:
                    von = variant[f"{call}_ms_r{k}"]
                    same = variant[f"clamped_r{k}"] == first[f"clamped_r{k}"]
                    lines.append(f"            the other build of the window ({VARIANT_NAME}): {f3(von)} ({von[0] / on[0]:.2f} x this build); pixels clamped {'the same' if same else 'DIFFER'}")
            if parent:
                a, b, c = off, second[f"{call}_ms_off"], parent[f"{call}_ms_off"]
                lo, hi = min(a[1], b[1]), max(a[2], b[2])
                ok = lo <= c[0] <= hi
                inside = inside and ok and parent["off_sha256"] == first["off_sha256"] == second["off_sha256"]
                lines.append(f"        clamp off, the parent commit's library in the same run: {f3(c)}; this build again: {f3(b)}; the parent's median is "
                             f"{'inside' if ok else 'OUTSIDE'} this build's spread [{lo:.3f}, {hi:.3f}]; images sha256 {parent['off_sha256']} / {first['off_sha256']}")
    lines += ["", f"condition (the whole call with the clamp on, guides cached, < the 32-spp batch it follows): worst share {100 * worst:.1f} % -> {'HELD' if worst < 1 else 'MISSED'}"]
    if parent_lib:
        lines.append(f"clamp off against the parent commit's library: {'every median inside the spread of this build, and the same images' if inside else 'NOT everywhere inside the spread (see above)'}")
    if os.path.exists(out_path):
        old = open(out_path).read().splitlines()
        at = [k for k, l in enumerate(old) if l.startswith(FOOT_RECORD)]
        if at:
            lines += [""] + old[at[0]:]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


GLASS_K = (0, 2, 4, 8)
GLASS_SCENES = (("room", 1), ("open", 0))


def quality_glass(out_path):
    """guides that follow glass (rpt_set_guides_through_glass) against first-hit guides, on the CPU: the host filters take guide arrays"""
    from oracle_ffi import Oracle
    import denoise_var_ref
    import guides_glass_ref
    import model_scenes
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    orc = Oracle("rpt_math")
    F = np.float32
    W = H = 128
    part = lambda img, ref, mask: float(np.linalg.norm((img.astype(np.float64) - ref)[mask]) / np.linalg.norm(ref.astype(np.float64)[mask]))
    planes = lambda g: (g["albedo"], g["normal"], g["position"], g["depth"], g["kind"])
    filters = (("rpt_denoise, defaults", lambda mean, g, m: hip.denoise_host(mean, *planes(g))),
               ("rpt_denoise_variance, defaults", lambda mean, g, m: hip.denoise_variance_host(mean, *planes(g), m)[0]),
               ("rpt_denoise_variance, sigma_variance 4", lambda mean, g, m: hip.denoise_variance_host(mean, *planes(g), m, hip.denoise_var_params(sigma_variance=4.0))[0]))
    lines = ["Guides that follow glass (rpt_set_guides_through_glass) against first-hit guides (tools/denoise_probe.py --quality-glass): the material-model scenes of",
             f"tests/model_scenes.py at {W} x {H}, the 8-spp mean of the restatement with models (tests/models_oracle) filtered by the host builds of the filters over the",
             "guides of tests/guides_glass_ref.py (K = 0: the first-hit guides), rel-L2 against the restatement's 1024-spp mean over (a) the pixels whose chain crossed glass",
             "and (b) the whole image.  K = max_interfaces.", ""]
    sums = {}
    for name, nee in GLASS_SCENES:
        t0 = time.time()
        world, rec, skybox, _ = model_scenes.scene(name)
        cfg = model_scenes.config(name, nee, W, H)
        sc = orc.scene(world, skybox_f32=skybox)
        rng = rpt.blue_noise_seeds(W, H)
        moments, noisy = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
        for _ in range(8):
            s, rng, _ = model_scenes.models_trace_cpu(cfg, sc, rec, rng, 1)
            denoise_var_ref.moments_add(moments, s[..., :3])
            noisy = (noisy + s).astype(F)
        rest, _, _ = model_scenes.models_trace_cpu(cfg, sc, rec, rng, 1024 - 8)
        conv = ((noisy[..., :3].astype(np.float64) + rest[..., :3]) / 1024.0)
        mean = (noisy[..., :3] / F(8)).astype(F)
        guides = {K: guides_glass_ref.guides(world, rec, K, cfg, orc, sc) for K in GLASS_K}
        finite = np.isfinite(mean).all(axis=-1) & np.isfinite(conv).all(axis=-1)      # (a sample that is not finite stays in both means: such pixels are left out)
        through = (guides[8][0]["interfaces"] > 0) & finite
        everything = finite
        info = guides[8][1]
        lines += [f"{name} (nee {nee}): {int(through.sum())} of {W * H} pixels look through glass ({int((~finite).sum())} pixels without a finite mean left out); rays per round at K = 8: {info['rays'][:info['rounds']]}; "
                  f"ended on glass at K = 2 / 4 / 8: {' / '.join(str(guides[K][1]['pixels_exhausted']) for K in (2, 4, 8))}",
                  f"  the 8-spp mean, unfiltered: (a) {part(mean, conv, through):.4f}  (b) {part(mean, conv, everything):.4f}"]
        for label, run in filters:
            row = []
            for K in GLASS_K:
                out = run(mean, guides[K][0], moments)
                ea, eb = part(out, conv, through), part(out, conv, everything)
                sums.setdefault((label, K), []).append(ea)
                row.append(f"K = {K}: (a) {ea:.4f} (b) {eb:.4f}")
            lines.append(f"  {label:40s} " + "   ".join(row))
        lines.append("")
        print(f"{name}: {time.time() - t0:.0f} s", flush=True)
    lines.append("summed (a) over the scenes:")
    best = None
    for label, _ in filters:
        lines.append(f"  {label:40s} " + "   ".join(f"K = {K}: {sum(sums[(label, K)]):.4f}" for K in GLASS_K))
    for K in GLASS_K[1:]:
        total = sum(sum(sums[(label, K)]) for label, _ in filters[:2])
        if best is None or total < best[0]:
            best = (total, K)
    lines += ["", f"lowest summed (a) of K = 2, 4, 8 over the two shipped-default filters: K = {best[1]} (hip.GUIDES_THROUGH_GLASS; the setting ships off)"]
    open(out_path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--quality-glass":
        quality_glass(a[1] if len(a) > 1 else os.path.join(ROOT, "profiles", "r20_glass_guides_quality.txt"))
    elif "--workload-firefly" in a:
        gpu_firefly_child(a[a.index("--workload-firefly") + 1])
    elif a and a[0] == "--gpu-firefly":
        gpu_firefly(a[1] if len(a) > 1 else os.path.join(ROOT, "profiles", "r16_firefly.txt"), os.environ.get("RPT_PARENT_LIB"), os.environ.get("RPT_VARIANT_LIB"))
    elif a and a[0] == "--quality-firefly":
        quality_firefly(a[1] if len(a) > 1 else os.path.join(ROOT, "profiles", "r16_firefly_quality.txt"))
    elif "--workload-temporal" in a:
        gpu_temporal_child(a[a.index("--workload-temporal") + 1])
    elif a and a[0] == "--gpu-temporal":
        gpu_temporal(a[1] if len(a) > 1 else os.path.join(ROOT, "profiles", "r15_temporal.txt"))
    elif a and a[0] == "--quality-temporal":
        quality_temporal(a[1] if len(a) > 1 else os.path.join(ROOT, "profiles", "r15_temporal_quality.txt"))
    elif "--workload-variance" in a:
        gpu_variance_child(a[a.index("--workload-variance") + 1])
    elif a and a[0] == "--gpu-variance":
        gpu_variance(a[1] if len(a) > 1 else os.path.join(ROOT, "profiles", "r14_denoise_variance.txt"))
    elif "--workload" in a:
        gpu_child(a[a.index("--workload") + 1])
    elif a and a[0] == "--quality":
        quality(a[1] if len(a) > 1 else os.path.join(ROOT, "profiles", "r11_denoise_quality.txt"))
    elif a and a[0] == "--quality-variance":
        quality_variance(a[1] if len(a) > 1 else os.path.join(ROOT, "profiles", "r14_denoise_variance_quality.txt"))
    elif a and a[0] == "--gpu":
        gpu(a[1] if len(a) > 1 else os.path.join(ROOT, "profiles", "r11_denoise.txt"))
    else:
        print(__doc__)
