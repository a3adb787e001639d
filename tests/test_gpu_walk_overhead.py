"""The streamed LDS walks after their loop head, addresses and LDS image were re-encoded (k_walk.h lds_walk_run, rpt_scene.hip build_lds_image: inner
descriptors are the pair index times four, one (a, e1, e2) record per triangle, the stack by its LDS address): every ray computes what it computed before.
Each image is held to the CPU oracle bit for bit through the production rpt_render, each ray count to the oracle's, each traced ray to the oracle's walk.

  * DarkCornell at 64 x 64, batches of 5, 32 and 33 samples on one context (known-length batches with several slots per pixel: FIRST, plain and LAST
    launches), both slot layouts, nee 0 and MIS (the shadow walks run the same loop);
  * FurnaceTest at 32 x 32 (walked from global memory: the kernels this change must leave alone);
  * a tree built by hand over 512 triangles at the extremes of the descriptor fields: a leaf of 63 triangles, a leaf whose first triangle is 511, and the
    deepest tree an LDS image takes (15 levels under the root: camera rays through the middle of the image stand 15 entries high on their stack);
  * rays on both sides of every bound of the exact-division guard (direction and origin components), a zero and a NaN component."""
import copy

import numpy as np
import pytest

import test_gpu_batch_seam as seam
import test_gpu_rcp_walks as rcp_walks

pytestmark = pytest.mark.gpu

BATCHES = (5, 32, 33)
_cache = {}


def _oracle_once(oracle, key, cfg, w, seeds, spp):
    """the oracle's (accumulators, statistics) for a case: computed once, never changed"""
    if key not in _cache:
        acc, _, st = oracle.trace_cpu(cfg, oracle.scene(w), seeds, spp)
        acc.setflags(write=False)
        _cache[key] = (acc, st)
    return _cache[key]


def _hold_to_oracle(acc, st, ref):
    acc_c, st_c = ref
    assert st["extension_rays"] == st_c.extension_rays and st["sky_evals"] == st_c.sky_evals and st["shadow_rays"] == st_c.shadow_rays
    differ = acc.view(np.uint32) != acc_c.view(np.uint32)
    assert not differ.any(), f"{int(differ.sum())} accumulator words differ"


@pytest.mark.parametrize("q_shift", [None, "3"])
@pytest.mark.parametrize("nee", [0, 1])
def test_darkcornell_batches_of_5_32_33(monkeypatch, hipmod, oracle, rpt, world, nee, q_shift):
    monkeypatch.delenv("RPT_LAST_ORDER", raising=False)
    if q_shift is None:
        monkeypatch.delenv("RPT_SLOT_Q_SHIFT", raising=False)
    else:
        monkeypatch.setenv("RPT_SLOT_Q_SHIFT", q_shift)
    w = world("DarkCornell")
    cfg = rpt.default_config(64, 64, nee=nee)
    seeds = rpt.blue_noise_seeds(64, 64)
    acc, st, _, last_walk = seam._render(hipmod, w, cfg, seeds, BATCHES)
    assert last_walk                                                   # the scene is LDS-resident and its last rays have a launch of their own
    _hold_to_oracle(acc, st, _oracle_once(oracle, ("darkcornell", nee), cfg, w, seeds, sum(BATCHES)))


@pytest.mark.parametrize("nee", [0, 1])
def test_furnace(hipmod, oracle, rpt, world, nee):
    w = world("FurnaceTest")
    cfg = rpt.default_config(32, 32, nee=nee)
    seeds = rpt.blue_noise_seeds(32, 32)
    acc, st, _, last_walk = seam._render(hipmod, w, cfg, seeds, (4,))
    assert not last_walk                                               # 10 240 triangles: no LDS image
    _hold_to_oracle(acc, st, _oracle_once(oracle, ("furnace", nee), cfg, w, seeds, 4))


# ---- the extremes of the descriptor fields -------------------------------------------------------------------------------------------------------------

LAYERS = 16                     # one leaf each; layer k (1 ..) lies in the plane z = 20 - k, the camera looks along +z from z = -3
LAYER_COUNTS = [63] + [32] * 14 + [1]
EXTREME_VIEW = dict(cam_position=(0.0, 0.0, -3.0, 0.0))


def extremes_scene(rpt):
    """512 triangles in 16 parallel layers and a node pool built by hand over them: a chain of 15 inner nodes, the left child of the i-th the leaf of layer
    i + 1, its right child the next inner node (the last one: the leaf of layer 16).  Leaves: 63 triangles, 14 x 32, and ONE triangle, index 511.  The layers
    nearer the camera are deeper in the chain, so a ray through all the boxes goes right at every node and pushes the left child: 15 entries."""
    if "extremes" in _cache:
        return _cache["extremes"]
    v, n, t = [], [], []
    rng = np.random.default_rng(5)
    for k in range(1, LAYERS + 1):
        z = 20.0 - k
        if k == LAYERS:
            i0 = len(v)
            v += [[-0.8, -0.6, z], [0.8, -0.6, z], [0.0, 0.9, z]]
            n += [[0.0, 0.0, -1.0]] * 3
            t += [[i0, i0 + 1, i0 + 2, 1]]
            continue
        nx, ny = (8, 4) if k == 1 else (4, 4)
        dx, dy = rng.uniform(-0.3, 0.3, 2)
        made = 0
        for i in range(nx):
            for j in range(ny):
                x0, y0 = -4.0 + 8.0 * i / nx + dx, -4.0 + 8.0 * j / ny + dy
                sx, sy = 0.75 * 8.0 / nx, 0.75 * 8.0 / ny
                mat = 3 if (k == 1 and i in (3, 4) and j == 3) else int((i + j + k) % 3)
                before = len(t)
                seam._quad(v, n, t, [(x0, y0, z), (x0 + sx, y0, z), (x0 + sx, y0 + sy, z), (x0, y0 + sy, z)], (0, 0, -1), mat)
                made += len(t) - before
        if k == 1:
            t.pop()                                                    # 64 -> 63
    assert len(t) == 512
    w = rpt.World.from_buffers(np.array(v, np.float32), np.array(n, np.float32), None, np.array(t, np.uint32), seam._materials(rpt, [9.0, 8.0, 7.0, 1.0]))
    # the builder put the triangles in ITS leaf order: back into layer order (stable), the light table's indices with them
    pos = w.per_vertex["vertex"][:, :3]
    layer = np.rint(20.0 - pos[w.indices["v0"], 2]).astype(np.int64)
    order = np.argsort(layer, kind="stable")
    inv = np.empty(512, np.int64)
    inv[order] = np.arange(512)
    w = copy.copy(w)
    w.indices = np.ascontiguousarray(w.indices[order])
    lp = w.light_pick.copy()
    lp["triangle_index_a"] = inv[lp["triangle_index_a"]]
    lp["triangle_index_b"] = inv[lp["triangle_index_b"]]
    w.light_pick = lp
    assert [int((np.sort(layer) == k).sum()) for k in range(1, LAYERS + 1)] == LAYER_COUNTS
    corners = np.stack([pos[w.indices[c]] for c in ("v0", "v1", "v2")], 1)                     # (512, 3, 3)
    first = np.concatenate([[0], np.cumsum(LAYER_COUNTS)[:-1]])
    lo = [corners[f:f + c].reshape(-1, 3).min(0) for f, c in zip(first, LAYER_COUNTS)]
    hi = [corners[f:f + c].reshape(-1, 3).max(0) for f, c in zip(first, LAYER_COUNTS)]
    nodes = np.zeros(2 * LAYERS - 1, w.nodes.dtype)

    def leaf(at, k):
        nodes[at] = (lo[k], LAYER_COUNTS[k], hi[k], first[k])

    for i in range(LAYERS - 1):                                        # inner node i: node 0, then the right child of the one before
        at = 0 if i == 0 else 2 * i
        nodes[at] = (np.min(lo[i:], 0), 0, np.max(hi[i:], 0), 2 * i + 1)
        leaf(2 * i + 1, i)
    leaf(2 * LAYERS - 2, LAYERS - 1)
    w.nodes = nodes
    w.bvh_max_depth = LAYERS - 1
    _cache["extremes"] = w
    return w


def test_the_extremes_scene_is_what_it_says(rpt):
    w = extremes_scene(rpt)
    leaves = w.nodes[w.nodes["triangle_count"] > 0]
    assert leaves["triangle_count"].max() == 63 and (leaves["left_or_first"] == 511).any() and len(w.nodes) == 31
    depth = {0: 0}
    for i, nd in enumerate(w.nodes):
        if nd["triangle_count"] == 0:
            depth[int(nd["left_or_first"])] = depth[int(nd["left_or_first"]) + 1] = depth[i] + 1
    assert max(depth.values()) == 15                                   # the deepest an LDS image takes (rpt_scene.hip stage_nodes)
    # a ray along the camera's axis is inside every box in x and y: both children are hit at each of the 15 inner nodes, and the right one (nearer) is entered
    assert (w.nodes["aabb_min"][:, :2] < -0.2).all() and (w.nodes["aabb_max"][:, :2] > 0.2).all()
    inner = w.nodes[w.nodes["triangle_count"] == 0]
    assert (w.nodes["aabb_min"][inner["left_or_first"] + 1, 2] < w.nodes["aabb_min"][inner["left_or_first"], 2]).all()


@pytest.mark.parametrize("nee", [0, 1])
def test_extremes_of_the_descriptor_fields(monkeypatch, hipmod, oracle, rpt, nee):
    monkeypatch.delenv("RPT_LAST_ORDER", raising=False)
    monkeypatch.delenv("RPT_SLOT_Q_SHIFT", raising=False)
    w = extremes_scene(rpt)
    cfg = rpt.default_config(64, 64, nee=nee, **EXTREME_VIEW)
    seeds = rpt.blue_noise_seeds(64, 64)
    acc, st, _, last_walk = seam._render(hipmod, w, cfg, seeds, (5, 8))
    assert last_walk                                                   # LDS-resident (the last rays' launch exists only there)
    ref = _oracle_once(oracle, ("extremes", nee), cfg, w, seeds, 13)
    assert ref[1].extension_rays > 64 * 64 * 13 * 1.2                  # paths go on between the layers (the bound tests/test_gpu_rcp_walks.py sets for its open room)
    _hold_to_oracle(acc, st, ref)


def test_extremes_ray_by_ray(hipmod, oracle, rpt):
    """rays from all around into the layers, through the production stage and the debug kernels (nearest and any hit): t, triangle and flags of each"""
    w = extremes_scene(rpt)
    rng = np.random.default_rng(8)
    n = 4096
    o = np.concatenate([rng.uniform(-5, 5, (n, 2)), rng.uniform(-4, 22, (n, 1))], 1).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[: n // 4] = (0.0, 0.0, 1.0)
    d[: n // 4, :2] += rng.normal(size=(n // 4, 2)).astype(np.float32) * np.float32(0.02)          # along the axis: all 15 levels
    o[: n // 4] = (0.0, 0.0, -3.0)
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        sc = oracle.scene(w)
        t_c, tri_c, fl_c, err = oracle.trace_rays(sc, 0, o, d)
        assert err == 0
        hit = (fl_c & 1) == 1
        assert n // 4 < hit.sum() < n and np.unique(tri_c[hit]).size > 300 and (tri_c[hit] & 0x7fffffff).max() == 511
        r.set_config(rpt.default_config(64, 64))
        r.reset(rpt.blue_noise_seeds(64, 64))
        t_p, tri_p, fl_p = r.debug_trace_rays_production(o, d)
        assert np.array_equal(fl_p, fl_c) and np.array_equal(t_p.view(np.uint32), t_c.view(np.uint32)) and np.array_equal(tri_p[hit], tri_c[hit])
        t_g, tri_g, fl_g = r.debug_trace_rays(False, o, d)
        assert np.array_equal(fl_g, fl_c) and np.array_equal(t_g.view(np.uint32), t_c.view(np.uint32)) and np.array_equal(tri_g[hit], tri_c[hit])
        max_t = (rng.random(n) * 12).astype(np.float32)
        _, _, afl_g = r.debug_trace_rays(True, o, d, max_t)
        _, _, afl_c, err = oracle.trace_rays(sc, 1, o, d, max_t)
        assert err == 0 and np.array_equal(afl_g & 1, afl_c & 1) and 0 < (afl_c & 1).sum() < n
    finally:
        r.close()


# ---- the exact-division guard ---------------------------------------------------------------------------------------------------------------------------

def guard_rays(w, n_each=24):
    """rays into DarkCornell with ONE component at, just inside and just outside a bound of the guard (csrc/rpt_fastdiv.h: direction |y| in [2^-40, 4),
    origin 0 or |v| in [2^-60, 2^40)), a zero, a denormal and a NaN in every component in turn, both signs; the other components random in the room"""
    rng = np.random.default_rng(31)
    f = np.float32

    def around(x):
        return [np.nextafter(f(x), f(0)), f(x), np.nextafter(f(x), f(np.inf))]

    d_edges = np.array(around(2.0 ** -40) + around(4.0) + [f(0.0), f(2.0 ** -130), f(np.nan)], f)
    o_edges = np.array(around(2.0 ** -60) + around(2.0 ** 40) + [f(0.0), f(2.0 ** -130), f(np.nan)], f)
    lo = w.per_vertex["vertex"][:, :3].min(axis=0)
    hi = w.per_vertex["vertex"][:, :3].max(axis=0)
    o, d = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for e in d_edges:
                dd = rng.normal(size=(n_each, 3)).astype(f)
                dd[:, axis] = f(sign) * e
                d.append(dd)
                o.append((lo + rng.random((n_each, 3)) * (hi - lo)).astype(f))
            for e in o_edges:
                oo = (lo + rng.random((n_each, 3)) * (hi - lo)).astype(f)
                oo[:, axis] = f(sign) * e
                o.append(oo)
                d.append(rng.normal(size=(n_each, 3)).astype(f))
    return np.concatenate(o), np.concatenate(d)


def test_rays_on_both_sides_of_the_division_guard(hipmod, oracle, rpt, world):
    w = world("DarkCornell")
    o, d = guard_rays(w)
    f = np.float32
    ad, ao = np.abs(d), np.abs(o)
    inside = ((ad >= f(2.0 ** -40)) & (ad < f(4.0))).all(axis=1) & ((ao == 0) | ((ao >= f(2.0 ** -60)) & (ao < f(2.0 ** 40)))).all(axis=1)
    assert inside.sum() > len(o) // 3 and (~inside).sum() > len(o) // 3        # both branches of the refill are taken, many times (NaN compares false: outside)
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        t_c, tri_c, fl_c, err = oracle.trace_rays(oracle.scene(w), 0, o, d)
        assert err == 0
        hit = (fl_c & 1) == 1
        assert hit[inside].sum() > 100 and hit[~inside].sum() > 100
        r.set_config(rpt.default_config(128, 128))
        r.reset(rpt.blue_noise_seeds(128, 128))
        t_p, tri_p, fl_p = r.debug_trace_rays_production(o, d)
        assert np.array_equal(fl_p, fl_c) and np.array_equal(t_p.view(np.uint32), t_c.view(np.uint32)) and np.array_equal(tri_p[hit], tri_c[hit])
        # the whole edge set of tests/test_gpu_rcp_walks.py through the same stage
        rcp_walks._edge_rays_against_the_oracle(r, oracle, rpt, w)
    finally:
        r.close()
