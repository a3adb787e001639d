#!/usr/bin/env python3
"""What punctual lights (rpt_set_punctual_lights; csrc/rpt_punctual.hip k_shade_punctual) cost, measured on one MI355X.

  python tools/punctual_lights_probe.py [out]       writes profiles/r23_punctual_lights.txt (or `out`), above the notes the file keeps at its foot
      --calls N      timed batches per setting (default 21)
      --small        128 x 128 images and 3 calls: a rehearsal of the code path, not a measurement (the file says so)

Per workload (DarkCornell 1024^2 and VeachMIS 1920 x 1080, both MIS, 32-spp batches) three settings alternate batch by batch in one process, after a warm-up
of each:
  current   no lights: k_shade, the kernels of a library without the feature
  forced    rpt_debug_force_punctual_kernels with no lights: k_shade_punctual, the same image (checked bit for bit before anything is timed); the ratio to
            current is the price of the switch
  lights    a point, a spot and a directional light placed from the scene's bounding box, pick_share 0.5: another image, other shadow rays — a record of
            what such a scene costs, not a comparison
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
SETTINGS = ("current", "forced", "lights")
FOOT = "---- notes (kept by tools/punctual_lights_probe.py) ----"


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return "%8.3f  [%8.3f .. %8.3f]" % (np.median(a), np.percentile(a, 10), np.percentile(a, 90))


def three_lights(hip, world):
    """a point light inside the upper half of the scene's box, a spot in an upper corner aimed at the centre, a directional light from above; intensities
    sized by the box so that the terms are of the order of 1"""
    p = world.per_vertex["vertex"][:, :3]
    lo, hi = p.min(0).astype(np.float64), p.max(0).astype(np.float64)
    c, e = (lo + hi) / 2, hi - lo
    d2 = float(np.dot(e, e)) / 4
    corner = c + e * (0.3, 0.35, -0.3)
    return hip.punctual_lights(hip.point_light(c + e * (-0.2, 0.25, 0.1), np.array((1.0, 0.9, 0.8)) * d2),
                               hip.spot_light(corner, c - corner, np.array((1.0, 1.0, 1.2)) * 2 * d2, 20.0, 35.0),
                               hip.directional_light((0.3, -1.0, 0.2), (0.6, 0.6, 0.5)))


def main():
    args = sys.argv[1:]
    small = "--small" in args
    calls = 3 if small else 21
    if "--calls" in args:
        calls = int(args[args.index("--calls") + 1])
    positional = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--calls")]
    out_path = positional[0] if positional else os.path.join(ROOT, "profiles", "r23_punctual_lights.txt")
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    lines = ["Punctual lights (rpt_set_punctual_lights): the current stage, the forced punctual variant with no lights, and three lights; one MI355X, tools/punctual_lights_probe.py",
             "median  [10th .. 90th percentile] over %d batches of %d spp per setting, the settings alternating batch by batch in one process; library %s" % (calls, SPP, hip.build_fingerprint()),
             "device %s" % (hip.device_info(0),)]
    if small:
        lines.append("REHEARSAL at 128 x 128 with %d calls: not a measurement" % calls)
    for scene, w, h in WORKLOADS:
        if small:
            w = h = 128
        world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
        cfg = rpt.default_config(w, h, nee=1)                    # (RPT_NEE_MIS)
        seeds = rpt.blue_noise_seeds(w, h)
        lights = three_lights(hip, world)
        contexts = {}
        for timing in (False, True):
            if timing:
                os.environ["RPT_STAGE_TIMING"] = "1"
            else:
                os.environ.pop("RPT_STAGE_TIMING", None)
            r = hip.Renderer(0)
            r.upload_scene(world); r.set_config(cfg); r.reset(seeds)
            contexts[timing] = r
        os.environ.pop("RPT_STAGE_TIMING", None)

        def setting(r, which):
            r.debug_force_punctual_kernels(which == "forced")
            r.set_punctual_lights(lights if which == "lights" else None, 0.5)

        try:
            images, variant = {}, {}
            for which in SETTINGS:                                   # warm-up of each, and the check that forced is current
                for r in contexts.values():
                    setting(r, which)
                    r.reset(seeds)
                    r.render(SPP)
                images[which] = contexts[False].read_accum()[0].copy()
                variant[which] = contexts[False].debug_last_shade_variant()
            assert variant == {"current": 0, "forced": 3, "lights": 3}, variant
            assert np.array_equal(images["current"].view(np.uint32), images["forced"].view(np.uint32)), scene + ": the forced variant's image is not the current stage's"
            assert not np.array_equal(images["current"], images["lights"]), scene + ": the lights changed nothing"
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
            lines.append("%s %d x %d, MIS, %d spp per batch; three lights (point, spot, directional), pick_share 0.5" % (scene, w, h, SPP))
            for what, label in (("batch", "32-spp batch, wall ms"), ("shade", "shade stage, kernel_ms")):
                lines.append("    %-26s current %s    forced %s    lights %s" % (label, stats(t[("current", what)]), stats(t[("forced", what)]), stats(t[("lights", what)])))
            lines.append("    forced / current: batch %.4f, shade stage %.4f" % (np.median(t[("forced", "batch")]) / np.median(t[("current", "batch")]),
                                                                                np.median(t[("forced", "shade")]) / np.median(t[("current", "shade")])))
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
