"""One process per rank (as `bench.py --gpus N` starts them) with the moments record and the counts flag inside the gather (rpt_gather_set_moments), over
tests/fake_rccl: three ranks render, then ONLY rank 1 renders a masked pass among its own pixels, and all gather again.  Rank 0's own counts are uniform
while the image's are not: the per-pixel-count decision of rpt_denoise_variance(RPT_DENOISE_GATHERED, NULL) has to come from rank 1's trailer — without it
the root divides every pixel by the uniform count and the last comparison fails.  Everything rank 0 reads is, bit for bit, what one context that did the
same sequence holds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = os.path.join(ROOT, "tests", "fake_rccl", "librccl_fake.so")
WORKER = os.path.join(ROOT, "tests", "fake_rccl", "gather_moments_worker.py")
W, H, WORLD, SAMPLES = 100, 70, 3, 4
MASK = (70, 10, 90, 30)                 # x0, y0, x1, y1: inside tile 1 (x 64..99, y 0..63), which rank 1 of 3 owns


def same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _env():
    env = dict(os.environ)
    env["RPT_RCCL_LIBRARY"] = FAKE
    env["RPT_FAKE_RCCL_TIMEOUT_S"] = "30"
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


def _unique_id():
    """rpt_comm_unique_id in a process of its own that resolves the stand-in (this pytest process may hold real RCCL)"""
    code = ("import importlib,sys; sys.path.insert(0, %r); hip = importlib.import_module('rust-path-tracer_amd.hip'); "
            "print(hip.comm_unique_id().hex()); print(hip.comm_library())" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=_env(), capture_output=True, text=True, timeout=120, check=True).stdout.split()
    assert out[1] == FAKE
    return out[0]


def _run_ranks(tmp_path):
    assert os.path.exists(FAKE), "tests/fake_rccl/librccl_fake.so is missing: make fake_rccl"
    uid = _unique_id()
    procs = []
    for rank in range(WORLD):
        log = open(tmp_path / f"rank{rank}.log", "w")
        cmd = [sys.executable, WORKER, "--uid", uid, "--rank", str(rank), "--world", str(WORLD), "--out", str(tmp_path), "--width", str(W), "--height", str(H),
               "--samples", str(SAMPLES), "--masked-rank", "1", "--mask", ",".join(map(str, MASK))]
        procs.append((subprocess.Popen(cmd, env=_env(), stdout=log, stderr=subprocess.STDOUT), log))
    failed = []
    for rank, (p, log) in enumerate(procs):
        try:
            rc = p.wait(timeout=120)
        except subprocess.TimeoutExpired:
            p.kill()
            rc = -9
        log.close()
        if rc != 0:
            failed.append((rank, rc, open(tmp_path / f"rank{rank}.log").read()[-2000:]))
    assert not failed, failed
    return [json.load(open(tmp_path / f"rank{r}.json")) for r in range(WORLD)]


def test_the_roots_count_decision_comes_from_the_other_ranks_trailers(hipmod, rpt, world, tmp_path):
    x0, y0, x1, y1 = MASK
    mask = np.zeros((H, W), np.uint8)
    mask[y0:y1, x0:x1] = 1
    xy = hipmod.tile_order(W, H, 1, WORLD)
    owned = np.zeros((H, W), bool)
    owned[xy >> 16, xy & 0xFFFF] = True
    assert owned[mask != 0].all() and not owned.all()
    # the one context that does the same sequence
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(world("DarkCornell"))
        r.set_config(rpt.default_config(W, H, nee=1))
        r.set_moments(True)
        r.reset(rpt.blue_noise_seeds(W, H))
        r.render(SAMPLES)
        r.render_pixels(mask, SAMPLES)
        acc, n = r.read_accum()
        acc, mom = acc.copy(), r.read_moments()
        rgb, var = r.denoise_variance(params=hipmod.denoise_var_params(iterations=3, sigma_variance=4.0), tonemap_op=3)
        assert n == SAMPLES and not r.counts_uniform()
    finally:
        r.close()
    infos = _run_ranks(tmp_path)
    assert sum(i["pixels"] for i in infos) == W * H and all(i["gather_moments"] for i in infos)
    assert [i["counts_uniform"] for i in infos] == [True, False, True]                    # the root's own counts are uniform ...
    root = infos[0]
    assert root["gathered_samples"] == SAMPLES
    assert root["gathered_info"] == {"with_moments": 1, "nonuniform": 1, "samples_min": SAMPLES, "samples_max": SAMPLES, "bad_trailers": 0}   # ... the image's are not
    assert same_bits(np.load(tmp_path / "image.npy"), acc)
    assert same_bits(np.load(tmp_path / "moments.npy"), mom)
    assert same_bits(np.load(tmp_path / "denoised.npy"), rgb) and same_bits(np.load(tmp_path / "variance.npy"), var)
