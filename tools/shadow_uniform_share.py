#!/usr/bin/env python3
"""Would the SHADOW walks of a mid-size scene become wave-uniform if their rays were dealt grouped by light?  (CPU analysis, no GPU.)

The any-hit walks of VeachMIS keep the texture-address unit 87 % busy (profiles/r04_veachmis_pmc_ta.txt) and are its dominant kernel.  The nearest-hit walks
got a scalar-cache path for wave-uniform node visits (k_walk.h children_uniform); shadow rays of a wave start on neighbouring surface points but aim at
RANDOM light triangles.  This replays the any-hit walks of the bounce-0 shadow rays of random 8 x 8 pixel blocks, S samples each, dealt to 64-lane waves
  slot    as the queue holds them today: a wave = the block at one sample index
  light   the block's S x 64 rays sorted by light-table index (the table follows triangle order: one emitter's triangles are contiguous), then cut into waves
and counts the inner steps in which all participating lanes stand on one node (one body per trip, majority rule, no refill).
usage: python tools/shadow_uniform_share.py [scene] [samples]
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from oracle_ffi import Oracle  # noqa: E402

rpt = importlib.import_module("rust-path-tracer_amd")
CASES = {"VeachMIS": (1920, 1080, {"nee": 1}), "FurnaceTest": (256, 256, {"nee": 1}), "DarkCornell": (1024, 1024, {"nee": 1})}


def replay(nl, ln, leaf):
    n = len(ln)
    pos = np.zeros(n, np.int64)
    inner = uniform = lanes = ulanes = 0
    cap = nl.shape[1]
    while True:
        act = pos < ln
        if not act.any():
            break
        cur = nl[np.arange(n), np.minimum(pos, cap - 1)]
        at_leaf = act & leaf[cur]
        at_inner = act & ~leaf[cur]
        if at_leaf.sum() > at_inner.sum():
            pos[at_leaf] += 1
            continue
        k = int(at_inner.sum())
        u = len(np.unique(cur[at_inner])) == 1
        inner += 1; lanes += k
        if u:
            uniform += 1; ulanes += k
        pos[at_inner] += 1
    return inner, uniform, lanes, ulanes


def main():
    scene = sys.argv[1] if len(sys.argv) > 1 else "VeachMIS"
    S = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    W, H, over = CASES[scene]
    orc = Oracle()
    w = rpt.World.from_path(rpt.fixture(scene + ".glb"))
    sc = orc.scene(w)
    cfg = rpt.default_config(W, H, **over)
    seeds = rpt.blue_noise_seeds(W, H)
    leaf = w.nodes.view(np.uint32).reshape(-1, 8)[:, 3] > 0
    sh = []
    for s in range(S):
        sd = seeds.copy()
        sd["n"] += s
        rays = np.zeros((W * H, 8), np.float32)
        valid = np.zeros(W * H, np.uint8)
        orc.lib.oracle_dump_shadow_rays(C.byref(cfg), C.byref(sc), sd.ctypes.data_as(C.c_void_p), C.c_uint32(0), rays.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p))
        sh.append((rays, valid))
    rng = np.random.default_rng(11)
    tot = {"slot": [0, 0, 0, 0], "light": [0, 0, 0, 0]}
    blocks = 0
    for _ in range(120):
        bx, by = int(rng.integers(0, W // 8)), int(rng.integers(0, H // 8))
        idx = np.array([(by * 8 + y) * W + bx * 8 + x for y in range(8) for x in range(8)])
        R = np.concatenate([sh[s][0][idx] for s in range(S)])
        V = np.concatenate([sh[s][1][idx] for s in range(S)]) == 1
        if V.sum() < 64:
            continue
        R = R[V]
        n = len(R)
        cap = 256
        nl = np.zeros((n, cap), np.uint32); ln = np.zeros(n, np.uint32)
        o = np.ascontiguousarray(R[:, :3]); d = np.ascontiguousarray(R[:, 3:6]); mt = np.ascontiguousarray(R[:, 6])
        orc.lib.oracle_trace_nodes(C.byref(sc), C.c_size_t(n), o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), mt.ctypes.data_as(C.c_void_p),
                                   nl.ctypes.data_as(C.c_void_p), C.c_uint32(cap), ln.ctypes.data_as(C.c_void_p))
        ln = np.minimum(ln, cap).astype(np.int64)
        for name, order in (("slot", np.arange(n)), ("light", np.argsort(R[:, 7], kind="stable"))):
            for a in range(0, n, 64):
                sel = order[a:a + 64]
                r = replay(nl[sel], ln[sel], leaf)
                for k in range(4):
                    tot[name][k] += r[k]
        blocks += 1
    print(f"{scene} {W}x{H}, bounce-0 shadow rays of {blocks} blocks x {S} samples:")
    for name, (inner, uniform, lanes, ulanes) in tot.items():
        print(f"  dealt by {name:5s}: inner trips wave-uniform {uniform / max(inner, 1):.1%} (of the lane-visits {ulanes / max(lanes, 1):.1%}); lanes per inner trip {lanes / max(inner, 1):.1f}; inner trips {inner}")


if __name__ == "__main__":
    main()
