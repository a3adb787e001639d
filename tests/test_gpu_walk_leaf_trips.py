"""The leaf trips of the streamed LDS walks (k_walk.h lds_stream_walk_run ONE_TRI, VOTE): in the plain nearest-hit launches a leaf trip tests ONE
triangle per lane, a lane whose leaf holds more stands on the rest of it — the descriptor (first + 1, count - 1) — until the next leaf trip, and a lane on a leaf
counts double in the vote; FIRST, LAST and the shadow kernels walk the whole leaf per trip beside it.  Per ray the tests, their order and every comparison are
unchanged, so everything here is the CPU oracle's bit for bit, on this library and on any earlier one.

  * a tree built by hand over 512 triangles, 16 leaves side by side under a balanced tree: leaves of 1, 2, 3, 17 and 63 triangles next to each other (a wave's rays
    stand on all of them at once; a lane in a leaf of 17 or 63 is in the middle of it when the 16-trip budget ends and the refill deals new rays to the lanes beside
    it), a leaf whose six triangles lie behind one another, the farthest first (every one is accepted, the nearest hit is the LAST triangle of the leaf), the same
    triangle twice in one leaf and once in each of two sibling leaves (the tie keeps the first tested), and a last leaf that ends at triangle 511;
  * one ray in seven has a zero direction component: outside the exact-division guard, it is walked alone by lds_walk_run in the same wave;
  * through PLAIN, FIRST and LAST (hit-or-miss lanes that accept in the middle of a leaf beside lanes that walk to the end), and through the four shadow kernels
    (near and fixed order, exact and segment-bounded) with bounds around the distance to the triangles;
  * the scene through rpt_render, and DarkCornell at 64 x 64 in batches of 5, 32 and 33 samples, both slot layouts, nee 0 and MIS."""
import copy

import numpy as np
import pytest

import test_gpu_batch_seam as seam
import test_gpu_walk_overhead as overhead
import test_gpu_walk_production as prod
from test_gpu_shadow_segment import sim  # noqa: F401  (the fixture: the CPU models of the exact and the segment rule)

pytestmark = pytest.mark.gpu

F = np.float32
COUNTS = [1, 2, 3, 17, 63, 6, 1, 1, 2, 63, 63, 63, 63, 63, 63, 38]     # leaf k = node 15 + k of a complete tree in heap order
FIRST_TRI = np.concatenate([[0], np.cumsum(COUNTS)[:-1]])
STACKED, TWIN_A, TWIN_B, DOUBLE = 5, 6, 7, 8                            # the leaves with a story; TWIN_A and TWIN_B are siblings (nodes 21 and 22)
PLANE_Z = 10.0
_cache = {}


def _leaf_triangles(k):
    """leaf k lives in the strip x in [k, k + 0.9], y in [0, 1] of the plane z = 10: as many slivers along y as it has triangles"""
    c, x0 = COUNTS[k], float(k)
    if k == TWIN_B:
        return _leaf_triangles(TWIN_A)                                  # the same triangle, in the sibling leaf
    if k == STACKED:                                                    # behind one another, the FARTHEST first: each is accepted, the last is the nearest
        return [[(x0, 0.0, PLANE_Z + 0.1 * (c - 1 - j)), (x0 + 0.9, 0.0, PLANE_Z + 0.1 * (c - 1 - j)), (x0, 0.9, PLANE_Z + 0.1 * (c - 1 - j))] for j in range(c)]
    if k == DOUBLE:
        return [[(x0, 0.0, PLANE_Z), (x0 + 0.9, 0.0, PLANE_Z), (x0, 0.9, PLANE_Z)]] * 2
    return [[(x0, j / c, PLANE_Z), (x0 + 0.9, j / c, PLANE_Z), (x0, (j + 0.9) / c, PLANE_Z)] for j in range(c)]


def leaf_scene(rpt):
    if "scene" in _cache:
        return _cache["scene"]
    assert sum(COUNTS) == 512 and len(COUNTS) == 16
    want = np.array([t for k in range(16) for t in _leaf_triangles(k)], F)                       # (512, 3, 3) in the order the leaves need
    leaf_of = np.repeat(np.arange(16), COUNTS)
    mats = np.where(np.arange(512) == 0, 3, (np.arange(512) + leaf_of) % 3)                      # ONE emitter: the triangle of the first leaf
    v = want.reshape(-1, 3)
    n = np.tile(np.array([[0, 0, -1]], F), (len(v), 1))
    t = np.stack([3 * np.arange(512), 3 * np.arange(512) + 1, 3 * np.arange(512) + 2, mats], 1).astype(np.uint32)
    w = rpt.World.from_buffers(v.copy(), n, None, t, seam._materials(rpt, [9.0, 8.0, 7.0, 1.0]))
    # the builder put the triangles in ITS leaf order: back into ours (equal triangles: in the order they come), the light table's indices with them
    pos = w.per_vertex["vertex"][:, :3]
    got = np.stack([pos[w.indices[c]] for c in ("v0", "v1", "v2")], 1)
    where = {}
    for i in range(512):
        where.setdefault(got[i].tobytes() + bytes([int(w.indices["material"][i])]), []).append(i)
    order = np.array([where[want[i].tobytes() + bytes([int(mats[i])])].pop(0) for i in range(512)])
    assert np.array_equal(np.sort(order), np.arange(512))
    inv = np.empty(512, np.int64)
    inv[order] = np.arange(512)
    w = copy.copy(w)
    w.indices = np.ascontiguousarray(w.indices[order])
    lp = w.light_pick.copy()
    lp["triangle_index_a"] = inv[lp["triangle_index_a"]]
    lp["triangle_index_b"] = inv[lp["triangle_index_b"]]
    w.light_pick = lp
    lo = [want[f:f + c].reshape(-1, 3).min(0) for f, c in zip(FIRST_TRI, COUNTS)]
    hi = [want[f:f + c].reshape(-1, 3).max(0) for f, c in zip(FIRST_TRI, COUNTS)]
    nodes = np.zeros(31, w.nodes.dtype)
    for k in range(16):
        nodes[15 + k] = (lo[k], COUNTS[k], hi[k], FIRST_TRI[k])
    for i in range(14, -1, -1):
        l, r = nodes[2 * i + 1], nodes[2 * i + 2]
        nodes[i] = (np.minimum(l["aabb_min"][:3], r["aabb_min"][:3]), 0, np.maximum(l["aabb_max"][:3], r["aabb_max"][:3]), 2 * i + 1)
    w.nodes = nodes
    w.bvh_max_depth = 4
    _cache["scene"] = w
    return w


def leaf_rays(origin=None, n=6144, seed=3):
    """rays towards points of the strips (and a little beside them); from all around in front of the plane, or all from `origin`.  One in seven has d.x == 0."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 16, n)
    target = np.stack([k + rng.uniform(-0.03, 0.93, n), rng.uniform(-0.05, 1.0, n), np.full(n, PLANE_Z)], 1)
    if origin is None:
        o = np.stack([rng.uniform(0, 16, n), rng.uniform(-1, 2, n), rng.uniform(-4, -2, n)], 1)
    else:
        o = np.tile(np.asarray(origin, np.float64), (n, 1))
    zero_x = np.arange(n) % 7 == 3
    if origin is None:
        o[zero_x, 0] = target[zero_x, 0]
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[zero_x, 0] = 0.0
    return np.ascontiguousarray(o, F), np.ascontiguousarray(d, F), zero_x


def test_the_leaf_scene_is_what_it_says(oracle, rpt):
    w = leaf_scene(rpt)
    leaves = w.nodes[w.nodes["triangle_count"] > 0]
    assert sorted(leaves["triangle_count"]) == sorted(COUNTS) and (leaves["left_or_first"] + leaves["triangle_count"]).max() == 512
    o, d, zero_x = leaf_rays()
    t, tri, fl, err = oracle.trace_rays(oracle.scene(w), 0, o, d)
    assert err == 0
    hit = (fl & 1) == 1
    tri = tri[hit] & 0x7fffffff
    leaf = np.searchsorted(FIRST_TRI, tri, side="right") - 1
    print(f"{int(hit.sum())} of {len(o)} rays hit; per leaf {np.bincount(leaf, minlength=16).tolist()}; {int(zero_x.sum())} rays outside the division guard")
    assert (np.bincount(leaf, minlength=16)[[k for k in range(16) if k != TWIN_B]] >= 32).all() and (~hit).sum() >= 32 and hit[zero_x].sum() >= 32
    assert np.unique(tri).size > 300 and tri.max() == 511
    assert (tri[leaf == STACKED] == FIRST_TRI[STACKED] + COUNTS[STACKED] - 1).sum() >= 32        # the nearest is the last of the leaf, behind up to five accepts
    assert not (leaf == TWIN_B).any() and (tri[leaf == DOUBLE] == FIRST_TRI[DOUBLE]).all()       # ties keep the first tested: the left leaf, the lower index
    # every wave of 64 consecutive rays stands on the thin and on the fat leaves
    for at in range(0, len(o), 64):
        ks = np.searchsorted(FIRST_TRI, tri_of_wave(fl, tri, hit, at), side="right") - 1
        assert (np.array(COUNTS)[ks] <= 3).any() and (np.array(COUNTS)[ks] >= 17).any()


def tri_of_wave(fl, tri_hit, hit, at):
    idx = np.flatnonzero(hit)
    sel = (idx >= at) & (idx < at + 64)
    return tri_hit[sel]


@pytest.mark.parametrize("q_shift", [None, "3"])
def test_plain_walk_ray_by_ray(monkeypatch, hipmod, oracle, rpt, q_shift):
    prod._env(monkeypatch, {} if q_shift is None else {"RPT_SLOT_Q_SHIFT": q_shift})
    w = leaf_scene(rpt)
    o, d, _ = leaf_rays()
    r = prod._renderer(hipmod, rpt, w)
    try:
        hit = prod._hold_nearest(r, hipmod.WALK_NEAREST_PLAIN, oracle, oracle.scene(w), o, d)
        assert 32 <= hit.sum() <= len(o) - 32
        for n in (1, 63, 65):                                                                     # fewer rays than a refill asks for idle lanes, and one wave and a bit
            prod._hold_nearest(r, hipmod.WALK_NEAREST_PLAIN, oracle, oracle.scene(w), o[100:100 + n], d[100:100 + n])
    finally:
        r.close()


@pytest.mark.parametrize("origin", [(7.6, 0.4, -3.0), (2.0, 0.5, 4.0), (15.25, 2.5, 9.0)], ids=["in front", "near", "grazing"])
def test_first_walk_ray_by_ray(monkeypatch, hipmod, oracle, rpt, origin):
    """every ray from the camera's position: the planes are staged with it subtracted, the triangle test keeps the true origin"""
    prod._env(monkeypatch, {})
    w = leaf_scene(rpt)
    o, d, _ = leaf_rays(origin=origin, seed=4)
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        r.set_config(rpt.default_config(64, 64, cam_position=(*origin, 0.0)))
        r.reset(rpt.blue_noise_seeds(64, 64))
        hit = prod._hold_nearest(r, hipmod.WALK_NEAREST_FIRST, oracle, oracle.scene(w), o, d)
        assert 32 <= hit.sum() <= len(o) - 32
    finally:
        r.close()


@pytest.mark.parametrize("mode", sorted(prod.parity.LAST_MODES))
def test_last_walk_ray_by_ray(monkeypatch, hipmod, oracle, rpt, mode):
    """hit-or-miss lanes leave at their first accepted triangle — in the middle of a leaf of 17 or 63, at the first of the six stacked ones — beside lanes that
    pass the emitter's test and walk every leaf to its end"""
    var, val, _ = prod.parity.LAST_MODES[mode]
    prod._env(monkeypatch, {var: val})
    w = leaf_scene(rpt)
    o, d, _ = leaf_rays(seed=5)
    o2, d2, _ = leaf_rays(origin=(0.3, 0.3, PLANE_Z - 6.0), n=1024, seed=6)                      # and rays from in front of the emitter: many pass its test
    d2[::2] = np.array([0.0, 0.0, 1.0], F) + np.random.default_rng(7).normal(size=(512, 3)).astype(F) * F(0.03)
    o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    r = prod._renderer(hipmod, rpt, w)
    try:
        lo = r.last_bounce_order()
        print(f"{mode}: {lo['mode_is']}, {lo['probe_rays']} probe rays")
        hit, may_emit, rest = prod._hold_last(r, hipmod, oracle, w, o, d, lo["mode"] != 0)
    finally:
        r.close()
    assert (may_emit & hit).sum() >= 32 and (~may_emit & hit).sum() >= 32 and (~hit).sum() >= 32
    assert (rest.sum() >= 32) == (lo["mode"] != 0)


@pytest.mark.parametrize("scene", ["leaves", "DarkCornell-near", "DarkCornell-fixed"])
def test_shadow_walks_ray_by_ray(monkeypatch, sim, hipmod, oracle, rpt, world, scene):  # noqa: F811
    """the shadow kernels (they keep the whole leaf per trip and the plain vote): any-hit rays that accept in the middle of a leaf or walk through it, exact and
    segment-bounded, on the leaf scene (no probe ray can be formed on it: the near order) and on DarkCornell in the near and in the fixed order"""
    order = scene.split("-")[1] if "-" in scene else "near"
    prod._env(monkeypatch, {"RPT_SHADOW_ORDER": order})
    if scene == "leaves":
        w = leaf_scene(rpt)
        o, d, _ = leaf_rays(seed=8)
        reach = (PLANE_Z - o[:, 2]) / np.where(d[:, 2] > 0, d[:, 2], 1)                           # the distance to the plane of the strips
        max_t = (reach * np.random.default_rng(9).uniform(0.6, 1.4, len(o))).astype(F)
    else:
        w = world("DarkCornell")
        o, d, max_t = prod.wr._shadow_like_rays(np.random.default_rng(10), 8000, w)
    exact, model = prod._shadow_refs(("leaf trips", scene.split("-")[0]), oracle, sim, oracle.scene(w), o, d, max_t)
    assert 0.05 * len(o) < exact.sum() < 0.95 * len(o)
    r = prod._renderer(hipmod, rpt, w)
    try:
        so = r.shadow_order()
        print(f"{scene}: fixed order {so['fixed']}, {so['probe_rays']} probe rays")
        assert so["fixed"] == (scene == "DarkCornell-fixed")
        prod._hold_shadow(r, hipmod, exact, model, o, d, max_t, shapes=(15, 65, 257))
    finally:
        r.close()


@pytest.mark.parametrize("nee", [0, 1])
def test_the_leaf_scene_through_rpt_render(monkeypatch, hipmod, oracle, rpt, nee):
    prod._env(monkeypatch, {})
    w = leaf_scene(rpt)
    cfg = rpt.default_config(32, 32, nee=nee, cam_position=(7.6, 0.4, -3.0, 0.0))
    seeds = rpt.blue_noise_seeds(32, 32)
    acc, st, _, last_walk = seam._render(hipmod, w, cfg, seeds, (5, 8))
    assert last_walk
    overhead._hold_to_oracle(acc, st, overhead._oracle_once(oracle, ("leaf trips", nee), cfg, w, seeds, 13))


@pytest.mark.parametrize("q_shift", [None, "3"])
@pytest.mark.parametrize("nee", [0, 1])
def test_darkcornell_batches_of_5_32_33(monkeypatch, hipmod, oracle, rpt, world, nee, q_shift):
    """FIRST, plain and LAST launches of known-length batches with several slots per pixel, and a batch of one more sample than a pixel has slots"""
    prod._env(monkeypatch, {} if q_shift is None else {"RPT_SLOT_Q_SHIFT": q_shift})
    w = world("DarkCornell")
    cfg = rpt.default_config(64, 64, nee=nee)
    seeds = rpt.blue_noise_seeds(64, 64)
    acc, st, _, last_walk = seam._render(hipmod, w, cfg, seeds, overhead.BATCHES)
    assert last_walk
    overhead._hold_to_oracle(acc, st, overhead._oracle_once(oracle, ("darkcornell", nee), cfg, w, seeds, sum(overhead.BATCHES)))
