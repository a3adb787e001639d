#!/usr/bin/env python3
"""What the thin-lens camera (rpt_set_camera_lens; csrc/rpt_lens.hip) costs, measured on one MI355X, and one picture with a visible focus plane.

  python tools/camera_lens_probe.py [out]       writes profiles/r21_camera_lens.txt (or `out`), above the notes the file keeps at its foot
      --calls N        timed batches per setting (default 21)
      --small          128 x 128 images and 3 calls: a rehearsal of the code path, not a measurement (the file says so)
      --picture PATH   also render PBRTest's wall of spheres, seen obliquely, 960 x 540, 256 spp, MIS, through a 55 degree lens focused on its middle, into PATH (PNG)

Per workload (DarkCornell 1024^2 and VeachMIS 1920 x 1080, both MIS, 32-spp batches) three settings alternate batch by batch in one process, after a
warm-up of each:
  default    the default record: the kernels of a library without the feature
  fov        tan_half_fov 0.6, no aperture: the full generate pass (k_generate_lens) against the FIRST walk that starts the paths itself
  aperture   tan_half_fov 1, aperture 0.05, focus at the scene's depth: the plain walk at bounce 0 and less coherent primary rays
The three render OTHER IMAGES with other ray counts: records, not a comparison.  Wall time of rpt_render (synchronised) and the rays it traced; median, and
the 10th and 90th percentile as the spread."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPP = 32
WORKLOADS = [("DarkCornell", 1024, 1024, 2.5), ("VeachMIS", 1920, 1080, 12.0)]      # (scene, width, height, focus distance of the aperture setting)
FOOT = "---- notes (kept by tools/camera_lens_probe.py) ----"


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return "%8.3f  [%8.3f .. %8.3f]" % (np.median(a), np.percentile(a, 10), np.percentile(a, 90))


def picture(rpt, hip, path):
    """PBRTest's wall of spheres seen obliquely, so that its columns lie at different depths: the camera is placed from the bounding box of everything above
    the ground, the plane in focus goes through the centre ray's first hit (the wall's middle), near and far columns and the ground blur"""
    import math
    w, h, spp, degrees = 960, 540, 256, 55
    world = rpt.World.from_path(rpt.fixture("PBRTest.glb"))
    p = world.per_vertex["vertex"][:, :3]
    above = p[p[:, 1] > 0.05]
    centre = 0.5 * (above.min(0) + above.max(0))
    pos = centre + np.array([-17.0, 0.5, -12.0])
    d = (centre - pos) / np.linalg.norm(centre - pos)
    cfg = rpt.default_config(w, h, nee=1, cam_position=tuple(float(v) for v in pos) + (0.0,), cam_rotation=(math.asin(-d[1]), math.atan2(d[0], d[2]), 0.0, 0.0))
    r = hip.Renderer(0)
    try:
        r.upload_scene(world)
        r.set_config(cfg)
        r.set_camera_lens(tan_half_fov=hip.tan_half_fov(degrees))
        r.reset(rpt.blue_noise_seeds(w, h))
        focus = float(r.guides()["depth"][h // 2, w // 2])             # the guides go through the lens centre: the centre ray's first hit
        r.set_camera_lens(tan_half_fov=hip.tan_half_fov(degrees), aperture_radius=0.025 * focus, focus_distance=focus)
        r.reset(rpt.blue_noise_seeds(w, h))
        for _ in range(spp // 32):
            r.render(32)
        rpt.host.write_png(path, r.resolve(3))
    finally:
        r.close()
    return "picture: PBRTest %d x %d, %d spp MIS, %d degree lens, camera (%.2f, %.2f, %.2f), aperture %.3f, focus %.3f (the centre ray's first hit) -> %s" % (
        w, h, spp, degrees, pos[0], pos[1], pos[2], 0.025 * focus, focus, os.path.basename(path))


def main():
    args = sys.argv[1:]
    small = "--small" in args
    calls = 3 if small else 21
    valued = ("--calls", "--picture")
    if "--calls" in args:
        calls = int(args[args.index("--calls") + 1])
    picture_path = args[args.index("--picture") + 1] if "--picture" in args else None
    positional = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] not in valued)]
    out_path = positional[0] if positional else os.path.join(ROOT, "profiles", "r21_camera_lens.txt")
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    lines = ["Thin-lens camera (rpt_set_camera_lens): the default record, a field of view, an aperture; one MI355X, tools/camera_lens_probe.py",
             "median  [10th .. 90th percentile] over %d batches of %d spp per setting, the settings alternating batch by batch in one process; library %s" % (calls, SPP, hip.build_fingerprint()),
             "device %s" % (hip.device_info(0),)]
    if small:
        lines.append("REHEARSAL at 128 x 128 with %d calls: not a measurement" % calls)
    for scene, w, h, focus in WORKLOADS:
        if small:
            w = h = 128
        world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
        cfg = rpt.default_config(w, h, nee=1)
        seeds = rpt.blue_noise_seeds(w, h)
        settings = {"default": None, "fov": hip.camera_lens(0.6, 0.0, 1.0), "aperture": hip.camera_lens(1.0, 0.05, focus)}
        r = hip.Renderer(0)
        try:
            r.upload_scene(world); r.set_config(cfg); r.reset(seeds)
            for which, lens in settings.items():                        # warm-up of each
                r.set_camera_lens(lens)
                r.render(SPP)
            t = {which: [] for which in settings}
            rays = {which: [] for which in settings}
            for _ in range(calls):
                for which, lens in settings.items():
                    r.set_camera_lens(lens)
                    before = r.stats()["extension_rays"]
                    t0 = time.perf_counter()
                    r.render(SPP)
                    t[which].append((time.perf_counter() - t0) * 1e3)
                    rays[which].append(r.stats()["extension_rays"] - before)
            lines.append("%s %d x %d, MIS, %d spp per batch; fov: tan_half_fov 0.6; aperture: radius 0.05, focus %.1f" % (scene, w, h, SPP, focus))
            for which in settings:
                ms = np.median(t[which])
                lines.append("    %-9s batch, wall ms %s    extension rays per batch %.4g    %.0f Mrays/s" % (which, stats(t[which]), np.median(rays[which]), np.median(rays[which]) / ms / 1e3))
        finally:
            r.close()
    if picture_path:
        lines.append(picture(rpt, hip, picture_path))
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
