#!/usr/bin/env python3
"""Time of the guides that follow glass (rpt_set_guides_through_glass) on one MI355X.

  python tools/glass_guides_probe.py [out]      per workload — the room and the open scene of tests/model_scenes.py at 1024 x 1024, DarkCornell 1024 x 1024 with one
                                                material made Glass — guides_ms (rpt_denoise_report, device events around the guide build) with the setting off and on
                                                (K = hip.GUIDES_THROUGH_GLASS), alternating in one process, median of 21 rebuilds each; the rays per round; and, on the
                                                room at 256 x 256, the share of pixels that find history in rpt_denoise_temporal after a camera move, off and on.
                                                RPT_PARENT_LIB = the parent commit's librpt_hip.so: its guides_ms (the setting does not exist there) from a process of
                                                its own, beside this build's with the setting off.  Writes profiles/r20_glass_guides.txt.
  python tools/glass_guides_probe.py --child NAME   one workload, one JSON line
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N, REPEATS = 1024, 21
WORKLOADS = ("room", "open", "DarkCornell")


def load(rpt, hip, name):
    """(world, records, skybox, configuration)"""
    if name == "DarkCornell":
        world = rpt.World.from_path(rpt.fixture("DarkCornell.glb"))
        quiet = [i for i in range(len(world.materials)) if not np.any(world.materials["emissive"][i, :3])]
        models = np.zeros(len(world.materials), np.uint32)
        models[quiet[-1]] = hip.MODEL_GLASS                   # the last material that does not emit
        return world, hip.material_models(models), None, rpt.default_config(N, N), int(quiet[-1])
    import model_scenes
    world, rec, skybox, _ = model_scenes.scene(name)
    return world, rec, skybox, model_scenes.config(name, 0, N, N), None


def child(name):
    import torch  # noqa: F401  (before the library: tests/conftest.py says why)
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    has_setting = hasattr(hip.lib(), "rpt_set_guides_through_glass")
    K = hip.GUIDES_THROUGH_GLASS
    world, rec, skybox, cfg, made_glass = load(rpt, hip, name)
    r = hip.Renderer(0)
    r.upload_scene(world, skybox_f32=skybox)
    r.set_material_models(rec)
    r.set_config(cfg)
    r.reset(rpt.blue_noise_seeds(N, N))
    r.render(1)
    resolve_only = hip.denoise_params(iterations=0)

    def rebuild(k):
        if has_setting:
            r.set_guides_through_glass(k)
        r.set_config(cfg)                                     # the same size: the accumulator stays, the guides are stale
        rep = r.denoise(params=resolve_only, with_report=True)[1]
        assert rep["guides_rebuilt"] == 1
        return rep["guides_ms"]

    for k in (0, K):
        rebuild(k)                                            # warm-up, both paths
    off, on = [], []
    for _ in range(REPEATS):
        off.append(rebuild(0))
        if has_setting:
            on.append(rebuild(K))
    out = {"name": name, "off": off, "on": on, "made_glass": made_glass, "pixels": N * N}
    if has_setting:
        out["info"] = r.guides_info()
        if name == "room":
            out["history"] = history_share(rpt, hip, r, K)
    r.close()
    print("RESULT " + json.dumps(out))


def history_share(rpt, hip, r, K, size=256):
    """pixels of view B that find history from view A (moved 0.2 sideways, yawed 0.05) in rpt_denoise_temporal at its defaults, setting off and on"""
    import model_scenes
    shares = {}
    a = model_scenes.config("room", 0, size, size)
    b = a.copy()
    b.cam_position[0] += 0.2
    b.cam_rotation[1] += 0.05
    r.set_moments(True)
    for k in (0, K):
        r.set_guides_through_glass(k)
        r.temporal_reset()
        for cfg in (a, b):
            r.set_config(cfg)
            r.reset(rpt.blue_noise_seeds(size, size))
            r.render(8)
            rep = r.denoise_temporal(with_report=True)[3]
        g = r.guides_info()
        shares[str(k)] = {"with_history": rep["pixels_with_history"], "pixels": size * size, "through_glass": g["pixels_through_glass"]}
    r.set_moments(False)
    return shares


def run_child(name, lib=None):
    env = dict(os.environ)
    if lib:
        env["RPT_HIP_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=env, capture_output=True, text=True, timeout=300)
    if p.returncode != 0:
        raise RuntimeError(f"{name}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main(out_path):
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    parent_lib = os.environ.get("RPT_PARENT_LIB")
    med = lambda v: float(np.median(v))
    lines = ["Guides that follow glass (rpt_set_guides_through_glass) on one MI355X (tools/glass_guides_probe.py): guides_ms of rpt_denoise_report — device events around",
             f"the guide build — with the setting off (first-hit guides) and on (K = {hip.GUIDES_THROUGH_GLASS}), alternating in one process, median of {REPEATS} rebuilds each [min, max];",
             f"{N} x {N}.  The expectation was about (1 + share of glass pixels x interfaces) walks; the rounds' rays say how many walks there were.", ""]
    for name in WORKLOADS:
        res = run_child(name)
        info = res["info"]
        n = res["pixels"]
        what = name + (f" (material {res['made_glass']} made Glass, ior 1.5)" if res["made_glass"] is not None else "")
        rays = info["rays"][:info["rounds"]]
        lines += [f"{what}: off {med(res['off']):.3f} ms [{min(res['off']):.3f}, {max(res['off']):.3f}]   on {med(res['on']):.3f} ms [{min(res['on']):.3f}, {max(res['on']):.3f}]"
                  f"   on / off {med(res['on']) / med(res['off']):.2f}",
                  f"  rays per round {rays} = {sum(rays) / n:.2f} walks of the image; {info['pixels_through_glass']} pixels ({100 * info['pixels_through_glass'] / n:.1f} %) look through glass, "
                  f"{info['pixels_exhausted']} end on glass"]
        if parent_lib:
            par = run_child(name, parent_lib)
            lo, hi = min(par["off"]), max(par["off"])
            m = med(res["off"])
            lines.append(f"  the parent commit's library: {med(par['off']):.3f} ms [{lo:.3f}, {hi:.3f}]; this build with the setting off, {m:.3f} ms, lies "
                         f"{'inside' if lo <= m <= hi else 'OUTSIDE'} that spread")
        if "history" in res:
            h = res["history"]
            lines.append("  rpt_denoise_temporal at its defaults, room 256 x 256, 8 spp per view, view B = view A moved 0.2 sideways and yawed 0.05: pixels that find history "
                         + ", ".join(f"K = {k}: {v['with_history']} of {v['pixels']} ({100 * v['with_history'] / v['pixels']:.1f} %)" for k, v in h.items())
                         + f"; {h[str(hip.GUIDES_THROUGH_GLASS)]['through_glass']} pixels of view B look through glass")
        lines.append("")
        print("\n".join(lines[-5:]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    open(out_path, "w").write("\n".join(lines))


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--child":
        child(a[1])
    else:
        main(a[0] if a else os.path.join(ROOT, "profiles", "r20_glass_guides.txt"))
