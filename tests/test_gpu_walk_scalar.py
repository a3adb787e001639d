"""The streamed LDS walks with their control flattened (k_walk.h lds_stream_walk_run, moller_trumbore_flat: one acceptance predicate in the place of four early-outs,
one pop site, a sentinel at the bottom of every stack column, one loop exit): every ray computes what it computed before.  Everything is held to the CPU oracle bit for
bit, and nothing here depends on which of the two forms the library was built with.

  * the predicate, ray by ray: two leaves over three triangles (one back-facing), rays in float32 ON the bounds of the triangle test — through the vertices, along the
    edges, at u + v == 1, around t = 0.001, |det| on both sides of 1e-6 —, and rays with a NaN or infinite component.  A float32 numpy restatement of the test sorts
    the rays into classes before the GPU is used;
  * empty and full stack columns side by side in a wave: rays that pop an empty column on their first or last trip, rays 15 entries high, rays that miss everything;
  * all seven kernels through rpt_render: the extremes scene of tests/test_gpu_walk_overhead.py in batches of 5 and 8 samples, nee 0 and MIS, both slot layouts, and once
    with segment-bounded shadow walks."""
import copy

import numpy as np
import pytest

import test_gpu_batch_seam as seam
import test_gpu_shadow_segment as segment
import test_gpu_walk_overhead as overhead
from test_gpu_shadow_segment import sim  # noqa: F401  (the fixture: the CPU model of the segment rule)

pytestmark = pytest.mark.gpu

F = np.float32
_cache = {}

# ---- the scene of the ray-by-ray tests: leaf A = (T0, T1), leaf B = (T2) ----------------------------------------------------------------------------------------
# T0 faces rays that travel along +z, T1 shows them its back, T2 faces them from a plane behind.  With dyadic coordinates and det = +-1 the barycentrics of a ray
# aimed at a dyadic point of the plane are computed without rounding: u and v land ON 0, and u + v ON 1.
TRIS = np.array([[(0, 0, 0), (0, 1, 0), (1, 0, 0)],          # T0: e1 = +y, e2 = +x: det = +d.z
                 [(2, 0, 1), (3, 0, 1), (2, 1, 1)],          # T1: e1 = +x, e2 = +y: det = -d.z (back-facing), one unit behind T0: leaf A's box has depth
                 [(4, 0, 2), (4, 1, 2), (5, 0, 2)]], F)      # T2: like T0


def two_leaf_scene(rpt):
    if "two" in _cache:
        return _cache["two"]
    v = TRIS.reshape(-1, 3)
    n = np.tile(np.array([[0, 0, -1]], F), (9, 1))
    t = np.array([[0, 1, 2, 0], [3, 4, 5, 1], [6, 7, 8, 3]], np.uint32)
    w = rpt.World.from_buffers(v.copy(), n, None, t, seam._materials(rpt, [9.0, 8.0, 7.0, 1.0]))
    pos = w.per_vertex["vertex"][:, :3]
    corners = np.stack([pos[w.indices[c]] for c in ("v0", "v1", "v2")], 1)                     # (3, 3, 3), in the builder's triangle order
    first_x = corners[:, 0, 0]
    order = np.argsort(first_x, kind="stable")                                                  # back into T0, T1, T2
    inv = np.empty(3, np.int64)
    inv[order] = np.arange(3)
    w = copy.copy(w)
    w.indices = np.ascontiguousarray(w.indices[order])
    lp = w.light_pick.copy()
    lp["triangle_index_a"] = inv[lp["triangle_index_a"]]
    lp["triangle_index_b"] = inv[lp["triangle_index_b"]]
    w.light_pick = lp
    corners = corners[order]
    assert np.array_equal(corners, TRIS)
    nodes = np.zeros(3, w.nodes.dtype)
    box = lambda c: (c.reshape(-1, 3).min(0), c.reshape(-1, 3).max(0))
    (alo, ahi), (blo, bhi), (rlo, rhi) = box(corners[:2]), box(corners[2:]), box(corners)
    nodes[0] = (rlo, 0, rhi, 1)
    nodes[1] = (alo, 2, ahi, 0)
    nodes[2] = (blo, 1, bhi, 2)
    w.nodes = nodes
    w.bvh_max_depth = 1
    _cache["two"] = w
    return w


def one_triangle_scene(rpt):
    if "one" in _cache:
        return _cache["one"]
    v = TRIS[0].copy()
    n = np.tile(np.array([[0, 0, -1]], F), (3, 1))
    w = rpt.World.from_buffers(v, n, None, np.array([[0, 1, 2, 3]], np.uint32), seam._materials(rpt, [9.0, 8.0, 7.0, 1.0]))
    _cache["one"] = w
    return w


# ---- the triangle test in float32, operation by operation (k_walk.h moller_trumbore; intersection.rs:9-54) ----------------------------------------------------------

def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1).astype(F)


def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(F) + a[:, 2] * b[:, 2]).astype(F)


def restate(o, d, tri):
    """the early-out each ray takes against its triangle (0 none, 1 |det| < 1e-6, 2 u, 3 v or u + v, 4 t < 0) and (det, u, v, t) as far as the test computes them"""
    o, d = o.astype(F), d.astype(F)
    a, e1, e2 = TRIS[tri, 0], (TRIS[tri, 1] - TRIS[tri, 0]).astype(F), (TRIS[tri, 2] - TRIS[tri, 0]).astype(F)
    with np.errstate(all="ignore"):
        pv = _cross(d, e2)
        det = _dot(e1, pv)
        inv = (F(1.0) / det).astype(F)
        tv = (o - a).astype(F)
        u = (_dot(tv, pv) * inv).astype(F)
        qv = _cross(tv, e1)
        v = (_dot(d, qv) * inv).astype(F)
        t = (_dot(e2, qv) * inv).astype(F)
        out = np.zeros(len(o), np.int64)
        out[(out == 0) & (np.abs(det) < F(1e-6))] = 1
        out[(out == 0) & ((u < 0) | (u > 1))] = 2
        out[(out == 0) & ((v < 0) | ((u + v).astype(F) > 1))] = 3
        out[(out == 0) & (t < 0)] = 4
    return out, det, u, v, t


def _dirs(rng, n):
    """dyadic directions with every component inside the exact-division guard: (k / 16, l / 16, 1), k and l odd or even but never 0"""
    k = rng.integers(1, 8, (n, 2)) * rng.choice([-1, 1], (n, 2))
    return np.concatenate([k / 16.0, np.ones((n, 1))], 1).astype(F)


def bound_rays():
    """(origins, directions, the triangle each ray is aimed at, the class it was built for)"""
    if "rays" in _cache:
        return _cache["rays"]
    rng = np.random.default_rng(22)
    o, d, tri, cls = [], [], [], []

    def aim(name, k, uv, s=2.0, scale=1.0):
        """rays through the point a + u e1 + v e2 of triangle k's plane, from s directions back (s < 0: from behind it, looking away)"""
        uv = np.asarray(uv, np.float64).reshape(-1, 2)
        a, e1, e2 = TRIS[k, 0].astype(np.float64), (TRIS[k, 1] - TRIS[k, 0]).astype(np.float64), (TRIS[k, 2] - TRIS[k, 0]).astype(np.float64)
        p = a + uv[:, :1] * e1 + uv[:, 1:] * e2
        dd = _dirs(rng, len(uv)).astype(np.float64)
        s = np.broadcast_to(np.asarray(s, np.float64).reshape(-1, 1), (len(uv), 1))
        o.append((p - s * dd).astype(F))
        d.append((dd * np.asarray(scale, np.float64).reshape(-1, 1)).astype(F))
        tri.append(np.full(len(uv), k))
        cls.extend([name] * len(uv))

    g = np.arange(1, 16) / 16.0
    for k in (0, 1, 2, 0, 1, 2):                                                           # (twice: other directions)
        aim("inside", k, [(x, y) for x in g[::3] for y in g[::3] if x + y < 1])
        aim("vertex", k, [(0, 0), (1, 0), (0, 1)] * 8)
        aim("u == 0", k, [(0, y) for y in g])
        aim("v == 0", k, [(x, 0) for x in g])
        aim("u + v == 1", k, [(x, 1 - x) for x in g])
        aim("u < 0", k, [(-1 / 64, y) for y in g[:12]])
        aim("u > 1", k, [(1 + 1 / 64, -y / 4) for y in g[:12]])
        aim("v < 0", k, [(x, -1 / 64) for x in g[:12]])
        aim("u + v > 1", k, [(x, 1 - x + 1 / 64) for x in g[:12]])
        aim("t < 0", k, [(x, y) for x in g[1::4] for y in g[1::4] if x + y < 1] * 2, s=-0.5)
        # t around 0.001: the distance to the plane a few floats either side of the constant
        near = F(0.001)
        steps = np.array([np.nextafter(near, F(0)), near, np.nextafter(near, F(1)), F(0.0009), F(0.0011), F(0.00099999), F(0.00100001)], np.float64)
        aim("t ~ 0.001", k, [(x, y) for x in g[2::4] for y in g[2:8:2] for _ in steps], s=np.tile(steps, 12))
        # |det| = |d.z| around 1e-6: the direction scaled, the plane a quarter away so that t stays below 1e6 where the determinant passes
        eps = F(1e-6)
        ladder = [eps]
        for _ in range(3):
            ladder = [np.nextafter(ladder[0], F(0))] + ladder + [np.nextafter(ladder[-1], F(1))]
        ladder = np.array(ladder, np.float64)
        pts = [(x, y) for x in g[2::4] for y in g[2:6:2]]
        for sign in (1.0, -1.0):
            aim("|det| ~ 1e-6", k, [p for p in pts for _ in ladder], s=np.tile(sign * 0.25 * np.ones(len(ladder)), len(pts)), scale=np.tile(sign * ladder, len(pts)))
    out = (np.concatenate(o), np.concatenate(d), np.concatenate(tri), np.array(cls))
    _cache["rays"] = out
    return out


def special_rays():
    """interior rays with ONE component of the origin or the direction NaN or +-inf"""
    o, d, tri, _ = bound_rays()
    pick = np.resize(np.flatnonzero(bound_rays()[3] == "inside"), 18 * 8).reshape(18, 8)
    o, d = o[pick.ravel()].copy().reshape(18, 8, 3), d[pick.ravel()].copy().reshape(18, 8, 3)
    row = 0
    for arr in (o, d):
        for axis in range(3):
            for val in (np.nan, np.inf, -np.inf):
                arr[row, :, axis] = val
                row += 1
    return o.reshape(-1, 3), d.reshape(-1, 3)


def test_the_rays_sit_on_the_bounds(oracle, rpt):
    """no GPU in here: the restatement's classes, and the oracle's agreement with it"""
    o, d, tri, cls = bound_rays()
    assert 1500 <= len(o) <= 2600
    out, det, u, v, t = restate(o, d, tri)
    for e in (1, 2, 3, 4):
        assert (out == e).sum() >= 32, (e, int((out == e).sum()))                      # every early-out is taken ...
    assert ((out == 0) | (out > 1)).sum() >= 32 and (out == 0).sum() >= 32             # ... and passed
    got = lambda m: int(m.sum())
    reach_u, reach_v = out != 1, (out == 0) | (out > 2)
    assert got(reach_u & (u == 0)) >= 32 and got(reach_v & (v == 0)) >= 32 and got(reach_v & ((u + v).astype(F) == 1)) >= 32
    assert got((cls == "vertex") & (out == 0)) >= 32
    assert got((out == 0) & (t > F(0.001))) >= 32 and got((out == 0) & (t >= 0) & ~(t > F(0.001))) >= 32
    around = cls == "|det| ~ 1e-6"
    assert got(around & (out == 1)) >= 32 and got(around & (out == 0)) >= 32 and got(around & (det < 0)) >= 32 and got(around & (det > 0)) >= 32
    # the oracle alone: a ray aimed at one triangle meets no other, so its answer is the restatement's
    w = two_leaf_scene(rpt)
    t_c, tri_c, fl_c, err = oracle.trace_rays(oracle.scene(w), 0, o, d)
    assert err == 0
    hit = (fl_c & 1) == 1
    accept = (out == 0) & (t > F(0.001)) & (t < F(1000000.0))
    assert np.array_equal(hit, accept), int((hit != accept).sum())
    assert np.array_equal(tri_c[hit] & 0x7fffffff, tri[hit]) and np.array_equal(t_c[hit].view(np.uint32), t[hit].view(np.uint32))
    assert np.array_equal((fl_c[hit] & 2) == 2, det[hit] < 0) and got(hit & (det < 0)) >= 32 and got(hit & (det > 0)) >= 32      # flag 2: the back of the triangle
    for name in ("t ~ 0.001", "|det| ~ 1e-6"):
        assert 32 <= got(hit & (cls == name)) <= got(cls == name) - 32, name          # both outcomes around a constant ...
    for on, off in (("u == 0", "u < 0"), ("v == 0", "v < 0"), ("u + v == 1", "u + v > 1"), ("vertex", "u > 1")):
        assert hit[cls == on].all() and not hit[cls == off].any()                     # ... and ON a bound the ray is in, one step past it out


def _hold_rays(r, oracle, sc, o, d, any_hit_bounds=True):
    t_c, tri_c, fl_c, err = oracle.trace_rays(sc, 0, o, d)
    assert err == 0
    hit = (fl_c & 1) == 1
    for t_g, tri_g, fl_g in (r.debug_trace_rays_production(o, d), r.debug_trace_rays(False, o, d)):
        assert np.array_equal(fl_g, fl_c) and np.array_equal(t_g.view(np.uint32), t_c.view(np.uint32)) and np.array_equal(tri_g[hit], tri_c[hit])
    bounds = [np.full(len(o), 2.0e6, F)]
    if any_hit_bounds:
        with np.errstate(all="ignore"):
            bounds += [t_c.copy(), np.nextafter(t_c, F(0)), np.nextafter(t_c, F(np.inf))]       # max_t on the hit, one float nearer, one farther
    answers = []
    for max_t in bounds:
        t_a, tri_a, fl_a, err = oracle.trace_rays(sc, 1, o, d, max_t)
        assert err == 0
        t_g, tri_g, fl_g = r.debug_trace_rays(True, o, d, max_t)
        occluded = (fl_a & 1) == 1
        assert np.array_equal(fl_g & 1, fl_a & 1)
        assert np.array_equal(t_g[occluded].view(np.uint32), t_a[occluded].view(np.uint32)) and np.array_equal(tri_g[occluded], tri_a[occluded])
        answers.append(occluded)
    return hit, answers


def test_the_predicate_ray_by_ray(hipmod, oracle, rpt):
    w = two_leaf_scene(rpt)
    o, d, _, _ = bound_rays()
    so, sd = special_rays()
    o, d = np.concatenate([o, so]), np.concatenate([d, sd])
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        r.set_config(rpt.default_config(64, 64))
        r.reset(rpt.blue_noise_seeds(64, 64))
        hit, answers = _hold_rays(r, oracle, oracle.scene(w), o, d)
    finally:
        r.close()
    assert np.array_equal(answers[0], hit) and np.array_equal(answers[1], hit)           # t <= max_t holds at max_t == t
    assert not answers[2][hit].all() and np.array_equal(answers[3], hit)                 # one float nearer the hit is lost (where t is not the leaf's only answer: never here)


# ---- empty and full stack columns ------------------------------------------------------------------------------------------------------------------------------

def test_empty_columns_on_the_first_and_the_last_trip(hipmod, oracle, rpt):
    """the two-leaf scene: rays that miss both children of the root pop an empty column on their first trip, rays that enter ONE leaf pop it on their last"""
    w = two_leaf_scene(rpt)
    rng = np.random.default_rng(9)
    n = 1024
    d = _dirs(rng, n)
    p = np.zeros((n, 3))
    p[:, 0] = np.where(np.arange(n) % 2 == 0, rng.uniform(0.1, 2.9, n), rng.uniform(7.0, 9.0, n))      # even: into leaf A's box; odd: past the root's box
    p[:, 1] = rng.uniform(0.1, 0.9, n)
    o = (p - 2.0 * d).astype(F)
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        r.set_config(rpt.default_config(64, 64))
        r.reset(rpt.blue_noise_seeds(64, 64))
        hit, _ = _hold_rays(r, oracle, oracle.scene(w), o, d, any_hit_bounds=False)
    finally:
        r.close()
    assert not hit[1::2].any() and 100 < hit[0::2].sum() < n // 2


def test_full_empty_and_dead_columns_side_by_side(hipmod, oracle, rpt):
    """the extremes scene: rays along the axis stand 15 entries high, their neighbours in the wave miss everything (a column that is never used) or end early"""
    w = overhead.extremes_scene(rpt)
    rng = np.random.default_rng(10)
    n = 2048
    o = np.tile(np.array([[0.0, 0.0, -3.0]], F), (n, 1))
    d = np.tile(np.array([[0.0, 0.0, 1.0]], F), (n, 1))
    d[:, :2] += rng.normal(size=(n, 2)).astype(F) * F(0.02)
    away = np.arange(n) % 3 == 1
    d[away] = rng.normal(size=(int(away.sum()), 3)).astype(F) * F([1, 1, 0.2]) + F([0, 0, -1])          # from the camera's side, looking back: nothing there
    short = np.arange(n) % 3 == 2
    o[short] = np.concatenate([rng.uniform(-4, 4, (int(short.sum()), 2)), rng.uniform(18.2, 18.8, (int(short.sum()), 1))], 1).astype(F)   # between the two deepest layers
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        r.set_config(rpt.default_config(64, 64))
        r.reset(rpt.blue_noise_seeds(64, 64))
        hit, _ = _hold_rays(r, oracle, oracle.scene(w), o, d, any_hit_bounds=False)
    finally:
        r.close()
    assert hit[~away & ~short].sum() > n // 4 and not hit[away].any()


def test_one_triangle(hipmod, oracle, rpt):
    w = one_triangle_scene(rpt)
    o, d, tri, _ = bound_rays()
    o, d = o[tri == 0], d[tri == 0]
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        r.set_config(rpt.default_config(64, 64))
        r.reset(rpt.blue_noise_seeds(64, 64))
        hit, _ = _hold_rays(r, oracle, oracle.scene(w), o, d)
    finally:
        r.close()
    assert 32 < hit.sum() < len(o) - 32


# ---- all seven kernels through the pipeline ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q_shift", [None, "3"])
@pytest.mark.parametrize("nee", [0, 1])
def test_extremes_through_every_streamed_kernel(monkeypatch, hipmod, oracle, rpt, nee, q_shift):
    """FIRST, plain and LAST walks (nee 0), both shadow orders (MIS: the scene has a flipped copy or not, as the upload decides), both slot layouts"""
    monkeypatch.delenv("RPT_LAST_ORDER", raising=False)
    if q_shift is None:
        monkeypatch.delenv("RPT_SLOT_Q_SHIFT", raising=False)
    else:
        monkeypatch.setenv("RPT_SLOT_Q_SHIFT", q_shift)
    w = overhead.extremes_scene(rpt)
    cfg = rpt.default_config(64, 64, nee=nee, **overhead.EXTREME_VIEW)
    seeds = rpt.blue_noise_seeds(64, 64)
    acc, st, _, last_walk = seam._render(hipmod, w, cfg, seeds, (5, 8))
    assert last_walk
    overhead._hold_to_oracle(acc, st, overhead._oracle_once(oracle, ("extremes", nee), cfg, w, seeds, 13))


@pytest.mark.parametrize("order", ["near", "fixed"])
def test_extremes_with_segment_bounded_shadow_walks(monkeypatch, sim, hipmod, oracle, rpt, order):
    """rpt_set_shadow_mode's segment mode on one context with the exact mode: the exact image is the oracle's bit for bit, the ray counts are equal, the segment image
    keeps the parity contract, and a pixel may differ from the exact one only where the CPU model of the rule loses an occlusion (tests/test_gpu_shadow_segment.py)"""
    monkeypatch.delenv("RPT_LAST_ORDER", raising=False)
    monkeypatch.delenv("RPT_SLOT_Q_SHIFT", raising=False)
    monkeypatch.setenv("RPT_SHADOW_ORDER", order)
    w = overhead.extremes_scene(rpt)
    cfg = rpt.default_config(64, 64, nee=1, **overhead.EXTREME_VIEW)
    seeds = rpt.blue_noise_seeds(64, 64)
    spp = 13
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        r.set_config(cfg)
        images, stats = {}, {}
        for mode in (hipmod.SHADOW_EXACT, hipmod.SHADOW_SEGMENT):
            r.set_shadow_mode(mode)
            r.reset(seeds)
            r.render_async(5)
            r.render_async(8)
            r.wait()
            images[mode] = r.read_accum()[0].copy()
            stats[mode] = r.stats()
    finally:
        r.close()
    ref = overhead._oracle_once(oracle, ("extremes", 1), cfg, w, seeds, spp)
    overhead._hold_to_oracle(images[hipmod.SHADOW_EXACT], stats[hipmod.SHADOW_EXACT], ref)
    ex, sg = images[hipmod.SHADOW_EXACT], images[hipmod.SHADOW_SEGMENT]
    se, ss = stats[hipmod.SHADOW_EXACT], stats[hipmod.SHADOW_SEGMENT]
    assert (ss["shadow_rays"], ss["extension_rays"]) == (se["shadow_rays"], se["extension_rays"]) and se["shadow_rays"] > 0
    assert segment.worst_pixel_rel_l2(sg, ref[0]) < segment.L2_BOUND
    where = np.argwhere((ex.view(np.uint32) != sg.view(np.uint32)).any(axis=2))
    print("pixels that differ between the modes:", len(where))
    if len(where):
        assert len(where) <= 64
        lost = segment._cpu_lost_occlusions(sim, cfg, oracle.scene(w), seeds, [int(y) << 16 | int(x) for (y, x) in where], spp)
        assert all((int(y) << 16 | int(x)) in lost for (y, x) in where)
