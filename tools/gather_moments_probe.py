#!/usr/bin/env python3
"""What the moments record inside the gather (rpt_gather_set_moments; csrc/k_gather.h) costs and saves, measured on one MI355X.

  python tools/gather_moments_probe.py [out]        writes profiles/r18_gather_moments.txt (or `out`), above the notes the file keeps at its foot
      --calls N      timed calls per setting and figure (default 21; at least 20)
      --small        128 x 128 images and 3 calls: a rehearsal of the code path, not a measurement (the file says so)

Per workload (DarkCornell 1024^2 and VeachMIS 1920 x 1080, both with NEE) and per driver — rpt_multi over 2, 4 and 8 ranks that SHARE the one device (the copy
transport of RPT_MULTI_ALLOW_SHARED_DEVICE), and one context with a local communicator — the two settings alternate call by call in the same process,
after a warm-up of both:
  (a) host wall time of rpt_multi_denoise_variance and rpt_multi_denoise_temporal (each returns synchronised).  Off is the host-merge path: a read-back of
      every rank's record, the merge, an upload.  On a local communicator off is what a process-per-GPU caller has to do without the setting:
      rpt_read_moments, then rpt_denoise_variance(RPT_DENOISE_GATHERED, that image); on is rpt_denoise_variance(RPT_DENOISE_GATHERED, NULL).
  (b) host wall time of a 32-spp rpt_multi_render + rpt_multi_wait (local: rpt_render_async + rpt_gather_async + rpt_gather_wait + rpt_wait): the price
      of the second record in the snapshot and the un-tile.
  (c) device_ms of the filter (device events around its kernels), as a check that it did not move.
Median, and the 10th and 90th percentile as the spread.  The results of the two settings are compared bit for bit before anything is timed.
Ranks that share a device say nothing about xGMI: the figures are the host's and the device's share of the work, not a link's."""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPP = 32
WORKLOADS = [("DarkCornell", 1024, 1024), ("VeachMIS", 1920, 1080)]
FOOT = "---- notes (kept by tools/gather_moments_probe.py) ----"


def stats(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return "%8.3f  [%8.3f .. %8.3f]" % (np.median(a), np.percentile(a, 10), np.percentile(a, 90))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def clock(call):
    t0 = time.perf_counter()
    out = call()
    return (time.perf_counter() - t0) * 1e3, out


def measure(name, set_setting, regather, forget, batch, variance, temporal, calls, lines):
    """the two settings alternating; variance / temporal return (..., report) with device_ms.  regather: what makes a gathered image exist again after a
    switch of the setting without rendering (rpt_multi does it by itself); forget: rpt_temporal_reset"""
    set_setting(False)
    batch()
    results = {}
    for setting in (False, True):                       # the same accumulators under both settings: what they return is compared, and both are warmed up
        set_setting(setting)
        regather()
        forget()
        results[setting] = (variance(), temporal())
        variance(); temporal()
    for k in (0, 1):
        assert all(same_bits(x, y) for x, y in zip(results[False][k][:2], results[True][k][:2])), name + ": the settings disagree"
    t = {(s, what): [] for s in (False, True) for what in ("batch", "variance", "variance_dev", "temporal", "temporal_dev")}
    for _ in range(calls):
        for setting in (False, True):
            set_setting(setting)
            batch()                                      # (the first batch after a switch sizes nothing: set_setting did)
            t[(setting, "batch")].append(clock(batch)[0])
            ms, out = clock(variance)
            t[(setting, "variance")].append(ms); t[(setting, "variance_dev")].append(out[-1]["device_ms"])
            ms, out = clock(temporal)
            t[(setting, "temporal")].append(ms); t[(setting, "temporal_dev")].append(out[-1]["device_ms"])
    lines.append("  %s" % name)
    for what, label in (("variance", "(a) denoise_variance, wall ms"), ("temporal", "(a) denoise_temporal, wall ms"), ("batch", "(b) 32-spp batch + gather, wall ms"),
                        ("variance_dev", "(c) denoise_variance, device_ms"), ("temporal_dev", "(c) denoise_temporal, device_ms")):
        lines.append("    %-36s off %s    on %s" % (label, stats(t[(False, what)]), stats(t[(True, what)])))


def main():
    args = sys.argv[1:]
    small = "--small" in args
    calls = 3 if small else 21
    if "--calls" in args:
        calls = int(args[args.index("--calls") + 1])
    positional = [a for i, a in enumerate(args) if not a.startswith("--") and (i == 0 or args[i - 1] != "--calls")]
    out_path = positional[0] if positional else os.path.join(ROOT, "profiles", "r18_gather_moments.txt")
    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    vp = hip.denoise_var_params()
    tp = hip.temporal_params()
    lines = ["The moments record inside the gather (rpt_gather_set_moments): setting off against on, one MI355X, tools/gather_moments_probe.py",
             "median  [10th .. 90th percentile] over %d calls per setting, the settings alternating call by call in one process; library %s" % (calls, hip.build_fingerprint()),
             "Ranks SHARE the one device (copy transport): nothing here says anything about xGMI.  device %s" % (hip.device_info(0),)]
    if small:
        lines.append("REHEARSAL at 128 x 128 with %d calls: not a measurement" % calls)
    for scene, w, h in WORKLOADS:
        if small:
            w = h = 128
        world = rpt.World.from_path(rpt.fixture(scene + ".glb"))
        cfg = rpt.default_config(w, h, nee=1)
        seeds = rpt.blue_noise_seeds(w, h)
        lines.append("%s %d x %d, NEE, %d spp per batch; the record is %.1f MB" % (scene, w, h, SPP, w * h * 16 / 1e6))
        for ranks in (2, 4, 8):
            m = hip.MultiRenderer([0] * ranks, allow_shared_device=True)
            try:
                m.upload_scene(world); m.set_config(cfg); m.set_moments(True); m.reset(seeds)

                def batch():
                    m.render(SPP)
                    m.wait()
                measure("rpt_multi, %d ranks on the one device" % ranks, m.gather_set_moments, lambda: None, m.temporal_reset, batch,
                        lambda: m.denoise_variance(params=vp, with_report=True), lambda: m.denoise_temporal(params=tp, with_report=True), calls, lines)
            finally:
                m.close()
        g = hip.Renderer(0)
        try:
            g.upload_scene(world); g.set_config(cfg); g.comm_init_local(); g.set_moments(True); g.reset(seeds)

            def batch():
                g.render_async(SPP)
                g.gather_async()
                g.gather_wait()
                g.wait()

            def image():
                return None if g.gather_moments() else g.read_moments()
            measure("one context, local communicator (off: rpt_read_moments + the image uploaded)", g.gather_set_moments, g.gather_async, g.temporal_reset, batch,
                    lambda: g.denoise_variance(source=hip.DENOISE_GATHERED, moments=image(), params=vp, with_report=True),
                    lambda: g.denoise_temporal(source=hip.DENOISE_GATHERED, moments=image(), params=tp, with_report=True), calls, lines)
        finally:
            g.close()
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
