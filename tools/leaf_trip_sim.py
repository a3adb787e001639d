#!/usr/bin/env python3
"""Analysis tool (CPU only): what a leaf trip of the streamed LDS walk should do, priced on the REAL leaves.
usage: tools/leaf_trip_sim.py [DarkCornell | extremes | <fixture name>] [--rays N] [--size W]

The oracle's event log (oracle_trace_events) says inner / leaf per visit but not how many triangles a leaf holds, so the reference's walk (intersection.rs:177-234,
intersect_front_to_back) is re-stated here in float32 numpy over World.nodes and World.indices, all rays in step; its visit kinds are compared with the oracle's log.
Rays: oracle_dump_rays at W x W, bounce 0 .. 3, dealt in slot order (8 x 8 pixel blocks), a wave owning 8 x 64 consecutive slots.
Replayed: the loop of k_walk.h lds_stream_walk_run — ONE body per trip, a look at the idle lanes every 16 trips, a refill at 16 or more idle lanes — with
    the leaf body    `whole`    every lane of the trip walks its whole leaf: the trip lasts as long as its longest leaf
                     `one`      one triangle per lane and trip; a lane with more stands on the rest of its leaf
                     `uniform`  triangles while EVERY lane of the trip has another one; lanes left over keep the rest
    the vote         a leaf trip iff weight x n_leaf > n_inner, weight 1, 2, 3
Costs in units of 3.7 per vector and 6.5 per scalar instruction (profiles/r04_valu_pipes.txt, question 3), from the static table of the plain kernel's `fast` walk
(tools/walk_overhead_count.py; COSTS below says which rows).  Per bounce and variant: units per ray, lanes per inner and per leaf trip, leaf trips per ray, and
the share of triangle iterations issued for fewer than eight lanes."""
import argparse
import ctypes as C
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle_ffi import Oracle  # noqa: E402

rpt = importlib.import_module("rust-path-tracer_amd")
hip = importlib.import_module("rust-path-tracer_amd.hip")

F = np.float32
# units = 3.7 VALU + 6.5 SALU of the rows of profiles/r25_leaf_trip_static_{parent,new}.txt, k_traverse_nearest_stream<16, 1024, 0>, walk `fast`
COSTS = dict(head=3 * 3.7 + 13 * 6.5,                 # loop head: paid by every trip
             inner=67 * 3.7 + 8 * 6.5 + 5 * 3.7 + 9 * 6.5,    # inner body + the share of push / pop (7 / 12) that is not the merged pop
             pop=2 * 3.7 + 3 * 6.5,                   # the merged pop site behind both bodies: paid by every trip
             setup=3 * 3.7 + 2 * 6.5,                 # leaf set-up of the looping forms (parent)
             tri_loop=73 * 3.7 + 15 * 6.5,            # one iteration of the triangle loop (parent)
             tri_one=74 * 3.7 + 12 * 6.5,             # the leaf body without a loop: set-up, test and the descriptor of the rest (new)
             tri_uniform=73 * 3.7 + 17 * 6.5,         # an iteration of a loop that ends on a ballot (an estimate: the parent's iteration + a ballot and a compare)
             refill=1200.0)
TRIPS, REFILL, SLOTS_PER_LANE = 16, 16, 8


def restate_walk(nodes, A, E1, E2, o, d, cap=256):
    """ev[ray, k] = 0 for an inner visit, the leaf's triangle count for a leaf visit; ln[ray] = visits"""
    n = len(o)
    count, left = nodes["triangle_count"].astype(np.int64), nodes["left_or_first"].astype(np.int64)
    lo, hi = nodes["aabb_min"][:, :3].astype(F), nodes["aabb_max"][:, :3].astype(F)
    cur, sp = np.zeros(n, np.int64), np.zeros(n, np.int64)
    stack = np.zeros((n, 32), np.int64)
    best = np.full(n, 1.0e6, F)
    live = np.ones(n, bool)
    ev, ln = np.zeros((n, cap), np.uint8), np.zeros(n, np.int64)

    def slab(node, idx):
        with np.errstate(all="ignore"):
            t1, t2 = (lo[node] - o[idx]) / d[idx], (hi[node] - o[idx]) / d[idx]
        tmin, tmax = np.fmin(t1[:, 0], t2[:, 0]), np.fmax(t1[:, 0], t2[:, 0])
        for k in (1, 2):
            tmin, tmax = np.fmax(tmin, np.fmin(t1[:, k], t2[:, k])), np.fmin(tmax, np.fmax(t1[:, k], t2[:, k]))
        return (tmax >= tmin) & (tmax > 0) & (tmin < best[idx]), tmin

    def pop(idx):
        empty = sp[idx] == 0
        live[idx[empty]] = False
        go = idx[~empty]
        sp[go] -= 1
        cur[go] = stack[go, sp[go]]

    cross = lambda a, b: np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F)
    dot = lambda a, b: ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(F) + a[:, 2] * b[:, 2]).astype(F)
    while live.any():
        idx = np.flatnonzero(live)
        c = count[cur[idx]]
        ev[idx, np.minimum(ln[idx], cap - 1)] = np.minimum(c, 255)
        ln[idx] += 1
        inner, leaf = idx[c == 0], idx[c > 0]
        if len(inner):
            l = left[cur[inner]]
            hit_l, tl = slab(l, inner)
            hit_r, tr = slab(l + 1, inner)
            with np.errstate(invalid="ignore"):
                swap = hit_r & (~hit_l | (tl > tr))
            both = hit_l & hit_r & (sp[inner] < 32)
            b = inner[both]
            stack[b, sp[b]] = np.where(swap[both], l[both], l[both] + 1)
            sp[b] += 1
            any_hit = hit_l | hit_r
            cur[inner[any_hit]] = np.where(swap[any_hit], l[any_hit] + 1, l[any_hit])
            pop(inner[~any_hit])
        if len(leaf):
            first, cnt = left[cur[leaf]], count[cur[leaf]]
            for k in range(int(cnt.max())):
                m = cnt > k
                i, t = leaf[m], first[m] + k
                with np.errstate(all="ignore"):
                    pv = cross(d[i], E2[t])
                    det = dot(E1[t], pv)
                    inv = (F(1.0) / det).astype(F)
                    tv = (o[i] - A[t]).astype(F)
                    u = (dot(tv, pv) * inv).astype(F)
                    qv = cross(tv, E1[t])
                    v = (dot(d[i], qv) * inv).astype(F)
                    tt = (dot(E2[t], qv) * inv).astype(F)
                    ok = ~(np.abs(det) < F(1e-6)) & ~(u < 0) & ~(u > 1) & ~(v < 0) & ~(u + v > 1) & ~(tt < 0) & (tt > F(0.001)) & (tt < best[i])
                best[i[ok]] = tt[ok]
            pop(leaf)
    assert ln.max() <= cap
    return ev, ln


def replay(ev, ln, form, weight):
    """the streamed loop over the rays in the order given; returns (units, inner trips, inner lanes, leaf trips, leaf lanes, triangle iterations, those under 8 lanes)"""
    n, span = len(ln), SLOTS_PER_LANE * 64
    units = 0.0
    it = il = lt = ll = iters = thin = 0
    for base in range(0, n, span):
        idx = [i for i in range(base, min(base + span, n)) if ln[i] > 0]
        nxt = 0
        ray, pos, rest = np.full(64, -1), np.zeros(64, np.int64), np.zeros(64, np.int64)      # rest: triangles left in the leaf the lane stands on
        while True:
            idle = np.flatnonzero(ray < 0)
            if nxt < len(idx) and len(idle) >= REFILL:
                take = idle[:len(idx) - nxt]
                ray[take] = idx[nxt:nxt + len(take)]
                pos[take] = 0
                rest[take] = ev[ray[take], 0]
                nxt += len(take)
                units += COSTS["refill"]
                continue
            if len(idle) == 64:
                break
            for _ in range(TRIPS if nxt < len(idx) else 1 << 30):
                live = ray >= 0
                if not live.any():
                    break
                at_leaf, at_inner = live & (rest > 0), live & (rest == 0)
                n_leaf, n_inner = int(at_leaf.sum()), int(at_inner.sum())
                units += COSTS["head"] + COSTS["pop"]
                if weight * n_leaf > n_inner:
                    lt += 1
                    ll += n_leaf
                    if form == "whole":
                        k = int(rest[at_leaf].max())
                        units += COSTS["setup"] + k * COSTS["tri_loop"]
                        for j in range(k):
                            lanes = int((rest[at_leaf] > j).sum())
                            iters += 1
                            thin += lanes < 8
                        done = at_leaf
                        rest[at_leaf] = 0
                    else:
                        k = 1 if form == "one" else int(rest[at_leaf].min())
                        units += k * COSTS["tri_one"] if form == "one" else COSTS["setup"] + k * COSTS["tri_uniform"]
                        iters += k
                        thin += k * (n_leaf < 8)
                        rest[at_leaf] -= k
                        done = at_leaf & (rest == 0)
                    step = done
                else:
                    it += 1
                    il += n_inner
                    units += COSTS["inner"]
                    step = at_inner
                pos[step] += 1
                end = step & (pos >= ln[np.maximum(ray, 0)])
                ray[end] = -1
                go = step & ~end
                rest[go] = ev[ray[go], pos[go]]
                rest[end] = 0
    return units, it, il, lt, ll, iters, thin


def scene_by_name(name):
    if name == "extremes":                       # the hand-built tree of tests/test_gpu_walk_overhead.py: leaves of 63, 14 x 32 and 1 triangles
        import test_gpu_walk_overhead as overhead
        return overhead.extremes_scene(rpt), overhead.EXTREME_VIEW
    return rpt.World.from_path(rpt.fixture(name + ".glb")), {}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", nargs="?", default="DarkCornell")
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--size", type=int, default=128)
    a = ap.parse_args()
    W = H = a.size
    orc = Oracle()
    w, view = scene_by_name(a.scene)
    sc = orc.scene(w)
    cfg = rpt.default_config(W, H, **view)
    seeds = rpt.blue_noise_seeds(W, H)
    order = hip.tile_order(W, H, 0, 1)
    px = (order >> 16).astype(np.int64) * W + (order & 0xFFFF).astype(np.int64)
    pos = w.per_vertex["vertex"][:, :3].astype(F)
    A = pos[w.indices["v0"]]
    E1, E2 = (pos[w.indices["v1"]] - A).astype(F), (pos[w.indices["v2"]] - A).astype(F)
    leaves = w.nodes[w.nodes["triangle_count"] > 0]["triangle_count"]
    print(f"{a.scene}: {len(w.nodes)} nodes, {len(w.indices)} triangles, leaves of 1 / 2 / more triangles: {int((leaves == 1).sum())} / {int((leaves == 2).sum())} / "
          f"{int((leaves > 2).sum())} (largest {int(leaves.max())})")
    print("costs: " + ", ".join(f"{k} {v:.1f}" for k, v in COSTS.items()))
    for bounce in range(4):
        rays, valid = np.zeros((W * H, 6), F), np.zeros(W * H, np.uint8)
        orc.lib.oracle_dump_rays(C.byref(cfg), C.byref(sc), seeds.ctypes.data_as(C.c_void_p), C.c_uint32(bounce), rays.ctypes.data_as(C.c_void_p),
                                 valid.ctypes.data_as(C.c_void_p))
        rays, valid = rays[px][:a.rays], valid[px][:a.rays]
        o, d = np.ascontiguousarray(rays[:, :3]), np.ascontiguousarray(rays[:, 3:])
        ev, ln = restate_walk(w.nodes, A, E1, E2, o, d)
        ln = np.where(valid == 1, ln, 0)
        ok = np.flatnonzero(valid == 1)
        if len(ok) < 64:
            print(f"bounce {bounce}: {len(ok)} rays — nothing to replay")
            continue
        kinds, kl = np.zeros((len(o), 256), np.uint8), np.zeros(len(o), np.uint32)
        orc.lib.oracle_trace_events(C.byref(sc), C.c_size_t(len(o)), o.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), kinds.ctypes.data_as(C.c_void_p),
                                    C.c_uint32(256), kl.ctypes.data_as(C.c_void_p))
        same = sum(int(kl[i] == ln[i] and np.array_equal(kinds[i, :ln[i]], (ev[i, :ln[i]] > 0).astype(np.uint8))) for i in ok)
        visits = np.concatenate([ev[i, :ln[i]] for i in ok])
        lv = visits[visits > 0]
        print(f"\nbounce {bounce}: {len(ok)} rays ({same} walk as the oracle's event log says), per ray {float((visits == 0).sum()) / len(ok):.1f} inner visits, "
              f"{len(lv) / len(ok):.2f} leaf visits, {float(lv.sum()) / len(ok):.2f} triangle tests; {100.0 * (lv > 1).mean():.1f} % of the leaf visits hold more than one triangle")
        print(f"  {'leaf body':8s} {'weight':>6s} {'units/ray':>10s} {'vs today':>9s} {'lanes/inner trip':>17s} {'lanes/leaf trip':>16s} {'leaf trips/ray':>15s} {'iterations < 8 lanes':>21s}")
        today = None
        for form in ("whole", "one", "uniform"):
            for weight in (1, 2, 3):
                u, it, il, lt, ll, iters, thin = replay(ev, ln, form, weight)
                today = u if today is None else today
                print(f"  {form:8s} {weight:6d} {u / len(ok):10.1f} {100.0 * (u / today - 1.0):+8.1f}% {il / max(it, 1):17.1f} {ll / max(lt, 1):16.1f} {lt / len(ok) * 64:15.2f}"
                      f" {100.0 * thin / max(iters, 1):20.1f}%")
    print("\n(leaf trips/ray: wave trips x 64 / rays — the trips a ray's wave spends in leaf bodies per ray it carries)")


if __name__ == "__main__":
    main()
