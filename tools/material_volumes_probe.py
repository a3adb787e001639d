#!/usr/bin/env python3
"""What absorbing glass (rpt_set_material_volumes; csrc/rpt_volumes.hip k_shade_volumes) costs, measured on one MI355X.

  python tools/material_volumes_probe.py [out]       writes profiles/r22_material_volumes.txt (or `out`), above the notes the file keeps at its foot
      --calls N      timed batches per setting (default 21)
      --small        128 x 128 images and 3 calls: a rehearsal of the code path, not a measurement (the file says so)

Per workload (DarkCornell 1024^2 and VeachMIS 1920 x 1080, both MIS, 32-spp batches, one object's material Glass with ior 1.5: the non-emissive material with
the most triangles) three settings alternate batch by batch in one process, after a warm-up of each:
  models    the model records alone: k_shade_models, the kernels of a library without the feature
  forced    rpt_debug_force_volume_kernels with all-zero volume records: k_shade_volumes, the same image (checked bit for bit before anything is timed); the
            ratio to models is the price of the variant itself
  volumes   the Glass material absorbs, sigma = absorption((0.6, 0.85, 0.7), half the object's extent): another image, another ray count (the roulette sees the
            attenuated throughput) — a record of what such a scene costs, not a comparison
Two contexts: one without stage timing gives the batch's wall time (rpt_render, synchronised), one with RPT_STAGE_TIMING=1 the shade stage's kernel_ms.
Median, and the 10th and 90th percentile as the spread."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPP = 32
WORKLOADS = [("DarkCornell", 1024, 1024), ("VeachMIS", 1920, 1080)]
COLOR = (0.6, 0.85, 0.7)
SETTINGS = ("models", "forced", "volumes")
FOOT = "---- notes (kept by tools/material_volumes_probe.py) ----"


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return "%8.3f  [%8.3f .. %8.3f]" % (np.median(a), np.percentile(a, 10), np.percentile(a, 90))


def choose_object(world):
    """(the object's material, the diagonal of its bounding box)"""
    mat = world.indices["material"]
    emissive = np.any(world.materials["emissive"][:, :3] != 0, axis=1)
    candidates = [m for m in range(len(world.materials)) if not emissive[m] and np.any(mat == m)]
    obj = max(candidates, key=lambda m: int((mat == m).sum()))
    t = world.indices[mat == obj]
    q = world.per_vertex["vertex"][:, :3][np.concatenate([t["v0"], t["v1"], t["v2"]])]
    return obj, float(np.linalg.norm(q.max(0) - q.min(0)))


def main():
    args = sys.argv[1:]
    small = "--small" in args
    calls = 3 if small else 21
    if "--calls" in args:
        calls = int(args[args.index("--calls") + 1])
    positional = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--calls")]
    out_path = positional[0] if positional else os.path.join(ROOT, "profiles", "r22_material_volumes.txt")
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    lines = ["Absorbing glass (rpt_set_material_volumes): the models variant, the forced volumes variant with all-zero records, and a Glass material that absorbs; one MI355X, tools/material_volumes_probe.py",
             "median  [10th .. 90th percentile] over %d batches of %d spp per setting, the settings alternating batch by batch in one process; library %s" % (calls, SPP, hip.build_fingerprint()),
             "device %s" % (hip.device_info(0),)]
    if small:
        lines.append("REHEARSAL at 128 x 128 with %d calls: not a measurement" % calls)
    for scene, w, h in WORKLOADS:
        if small:
            w = h = 128
        world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
        cfg = rpt.default_config(w, h, nee=1)
        seeds = rpt.blue_noise_seeds(w, h)
        obj, extent = choose_object(world)
        rec = hip.material_models([hip.MODEL_PBR] * len(world.materials))
        rec["model"][obj] = hip.MODEL_GLASS
        zeros = hip.material_volumes(np.zeros((len(world.materials), 3)))
        vols = zeros.copy()
        vols["sigma"][obj] = hip.absorption(COLOR, 0.5 * extent)
        contexts = {}
        for timing in (False, True):
            if timing:
                os.environ["RPT_STAGE_TIMING"] = "1"
            else:
                os.environ.pop("RPT_STAGE_TIMING", None)
            r = hip.Renderer(0)
            r.upload_scene(world); r.set_material_models(rec); r.set_config(cfg); r.reset(seeds)
            contexts[timing] = r
        os.environ.pop("RPT_STAGE_TIMING", None)

        def setting(r, which):
            r.debug_force_volume_kernels(which == "forced")
            r.set_material_volumes({"models": None, "forced": zeros, "volumes": vols}[which])

        try:
            images, variant = {}, {}
            for which in SETTINGS:                                   # warm-up of each, and the check that forced is models
                for r in contexts.values():
                    setting(r, which)
                    r.reset(seeds)
                    r.render(SPP)
                images[which] = contexts[False].read_accum()[0].copy()
                variant[which] = contexts[False].debug_last_shade_variant()
            assert variant == {"models": 1, "forced": 2, "volumes": 2}, variant
            assert np.array_equal(images["models"].view(np.uint32), images["forced"].view(np.uint32)), scene + ": the forced variant's image is not the models variant's"
            assert not np.array_equal(images["models"], images["volumes"]), scene + ": the absorbing material changed nothing"
            t = {(which, what): [] for which in SETTINGS for what in ("batch", "shade")}
            for _ in range(calls):
                for which in SETTINGS:
                    r = contexts[False]
                    setting(r, which)
                    t0 = time.perf_counter()
                    r.render(SPP)
                    t[(which, "batch")].append((time.perf_counter() - t0) * 1e3)
                    r = contexts[True]
                    setting(r, which)
                    before = r.stats()["kernel_ms"]["shade"]
                    r.render(SPP)
                    t[(which, "shade")].append(r.stats()["kernel_ms"]["shade"] - before)
            lines.append("%s %d x %d, MIS, %d spp per batch; material %d of %d Glass (ior 1.5), sigma %s = absorption(%s, %.4g)"
                         % (scene, w, h, SPP, obj, len(world.materials), tuple(float("%.4g" % s) for s in vols["sigma"][obj]), COLOR, 0.5 * extent))
            for what, label in (("batch", "32-spp batch, wall ms"), ("shade", "shade stage, kernel_ms")):
                lines.append("    %-26s models %s    forced %s    volumes %s" % (label, stats(t[("models", what)]), stats(t[("forced", what)]), stats(t[("volumes", what)])))
            lines.append("    forced / models: batch %.4f, shade stage %.4f" % (np.median(t[("forced", "batch")]) / np.median(t[("models", "batch")]),
                                                                               np.median(t[("forced", "shade")]) / np.median(t[("models", "shade")])))
        finally:
            for r in contexts.values():
                r.close()
    foot = []
    if os.path.exists(out_path):
        old = open(out_path).read().split("\n")
        if FOOT in old:
            foot = old[old.index(FOOT):]
    with open(out_path, "w") as f:
        f.write("\n".join(lines + foot) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
