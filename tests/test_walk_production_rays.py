"""The ray sets of tests/walk_rays.py, without a GPU: they sit where they are meant to sit, the oracle agrees with their float32 restatement, and they can tell the
reference's walk from a nearly right one — for each of seven comparisons a production walk kernel could get wrong (walk_rays.NEAR_MISSES) at least 32 rays of
the sets change their answer.  That stands in the place of planting wrong kernels on a GPU: tests/test_gpu_walk_production.py sends these very rays through
every walk rpt_render launches and holds each answer to the oracle."""
import ctypes as C

import numpy as np
import pytest

import walk_rays as wr
from oracle_ffi import _p
from test_anyhit_order import sim  # noqa: F401  (the fixture: tools/anyhit_order_sim.cpp, the CPU models of the exact and the segment rule)

F = np.float32
ENOUGH = 32


def _unique(d):
    keep = np.zeros(len(d), bool)
    keep[np.unique(d, axis=0, return_index=True)[1]] = True
    return keep


@pytest.fixture(scope="module")
def two_leaf(oracle, rpt):
    w = wr.two_leaf_scene(rpt)
    return w, oracle.scene(w)


@pytest.fixture(scope="module")
def ladder(oracle, two_leaf):
    """the ladder's rays, the oracle's nearest hits of them, and per rung (max_t, the oracle's occluded bit): computed once, never changed"""
    o, d, tri, cls = wr.ladder_rays()
    t, hit_tri, flags, err = oracle.trace_rays(two_leaf[1], 0, o, d)
    assert err == 0
    rungs = {}
    for rung, max_t in wr.shadow_bounds(t):
        _, _, fl, err = oracle.trace_rays(two_leaf[1], 1, o, d, max_t)
        assert err == 0
        rungs[rung] = (max_t, (fl & 1) == 1)
    return o, d, tri, cls, t, hit_tri, flags, rungs


def test_every_rung_of_the_ladder_separates_what_it_is_for(ladder):
    o, d, tri, cls, t, _, flags, rungs = ladder
    hit = (flags & 1) == 1
    assert len(o) <= 2600 and hit.sum() >= 500 and (~hit).sum() >= 500
    count = {r: (int((occ & hit).sum()), int((~occ & hit).sum()), int(occ[~hit].sum())) for r, (_, occ) in rungs.items()}
    print(count)
    assert list(rungs) == list(wr.RUNGS) and set(wr.UNBOUNDED) | set(wr.NOTHING) < set(wr.RUNGS)
    for r in wr.RUNGS:
        assert count[r][2] == 0, r                                         # a ray with no hit is occluded under no bound
    for r in ("t", "t+", "1e6-") + wr.UNBOUNDED:
        assert count[r][0] == hit.sum() >= ENOUGH, r                       # the bound is on or behind the hit: every hit occludes
    for r in ("t-",) + wr.NOTHING:
        assert count[r][1] == hit.sum() >= ENOUGH and count[r][0] == 0, r  # one float nearer, NaN, at or below 0.001: none does
    # the float above 0.001 is the one bound between the two: it keeps the hits AT that float and loses every other one
    assert count["0.001+"][0] >= ENOUGH and count["0.001+"][1] >= ENOUGH
    above = np.nextafter(wr.EPS, F(1))
    assert np.array_equal(rungs["0.001+"][1], hit & (t == above)) and (hit & (cls == "t == 0.001+")).sum() >= ENOUGH
    # the three classes the ladder adds to bound_rays(): t == 0.001 to the bit is no hit, and neither is a triangle passed at t >= 1e6
    for name in ("t == 0.001", "t >= 1e6"):
        assert (cls == name).sum() >= ENOUGH and not hit[cls == name].any(), name
    _, _, _, _, t_own = wr.restate(o, d, tri)
    assert np.all(t_own[cls == "t == 0.001"] == wr.EPS) and np.all(t_own[cls == "t >= 1e6"] >= wr.FAR)
    assert (wr.restate(o, d, tri)[0][cls == "t >= 1e6"] == 0).all()        # (they pass the triangle's own test)


@pytest.mark.parametrize("origin", sorted(wr.FAN_ORIGINS))
def test_every_class_of_the_fan_holds_both_outcomes(origin):
    """From a common origin the classes are computed, not constructed.  "just inside" and "just outside" must hold 32 rays each that pass, and fail, the test of the
    triangle they are aimed at; rays aimed AT a vertex or an edge fall to either side as the rounding has it: the counts are printed, 32 of each outcome are required
    where the geometry gives them, and where it does not the two neighbouring classes stand in (they are required whatever the count)."""
    o, d, tri, cls = wr.two_leaf_fan(origin)
    assert np.all(o == o[0]) and len(o) <= 4000
    keep = _unique(d)
    passes = wr.restate(o, d, np.where(tri >= 0, tri, 0))[0] == 0
    hit = wr.walk_two_leaf(o, d)[0]
    n = lambda m: int((m & keep).sum())
    assert n((cls == "just inside") & passes) >= ENOUGH and n((cls == "just outside") & ~passes) >= ENOUGH
    assert n((cls == "just inside") & ~passes) == 0 and n((cls == "just outside") & passes) == 0
    for name in ("vertex", "edge"):
        inside, outside = n((cls == name) & passes), n((cls == name) & ~passes)
        print(f"{origin}: {name}: {inside} rays pass the aimed triangle's test, {outside} fail it" + ("" if min(inside, outside) >= ENOUGH else
              f" — fewer than {ENOUGH} of one outcome: 'just inside' and 'just outside' stand in"))
        assert inside + outside >= ENOUGH and inside > 0 and outside > 0
    assert n((cls == "edge") & passes) >= ENOUGH and n((cls == "edge") & ~passes) >= ENOUGH
    assert n((cls == "random") & hit) >= ENOUGH and n((cls == "random") & ~hit) >= ENOUGH, (n((cls == "random") & hit), n((cls == "random") & ~hit))
    # the origins are what they are called
    lo, hi = wr.TRIS.reshape(-1, 3).min(0), wr.TRIS.reshape(-1, 3).max(0)
    inside_root = bool(np.all((o[0] > lo) & (o[0] < hi)))
    assert inside_root == (origin == "inside")
    if origin == "far":
        planes = np.stack([b for box in wr._LEAF_BOXES for b in box])
        assert np.linalg.norm(o[0]) > 1e4 and np.any((planes - o[0]).astype(F).astype(np.float64) != planes.astype(np.float64) - o[0].astype(np.float64))   # plane - origin rounds
    if origin == "on a box plane":
        assert any(np.any(o[0] == b) for box in wr._LEAF_BOXES for b in box) and np.all(o[0] != 0)
    if origin == "zero coordinate":
        assert np.any(o[0] == 0)


def test_the_oracle_agrees_with_the_restatement(oracle, two_leaf, ladder):
    """kinds 0 and 1 of oracle.trace_rays against walk_rays.walk_two_leaf — boxes, order, triangle tests and acceptance in float32 numpy — on every ray of the sets"""
    sc = two_leaf[1]
    o, d, _, _, t, hit_tri, flags, rungs = ladder
    sets = [("ladder", o, d, t, hit_tri, flags)]
    for name in wr.FAN_ORIGINS:
        fo, fd, _, _ = wr.two_leaf_fan(name)
        ft, ftri, ffl, err = oracle.trace_rays(sc, 0, fo, fd)
        assert err == 0
        sets.append((name, fo, fd, ft, ftri, ffl))
    for name, so, sd, t_c, tri_c, fl_c in sets:
        hit, best, tri, back = wr.walk_two_leaf(so, sd)
        assert np.array_equal(hit, (fl_c & 1) == 1), name
        assert np.array_equal(best.view(np.uint32), t_c.view(np.uint32)), name
        assert np.array_equal(tri[hit], tri_c[hit]) and np.array_equal(back[hit], (fl_c[hit] & 2) == 2), name
        bounds = wr.shadow_bounds(t_c)
        for rung, max_t in bounds:
            if name == "ladder":
                occluded = rungs[rung][1]
            else:
                _, _, fl, err = oracle.trace_rays(sc, 1, so, sd, max_t)
                assert err == 0
                occluded = (fl & 1) == 1
            assert np.array_equal(wr.walk_two_leaf(so, sd, max_t), occluded), (name, rung)
    # restate_triangle is restate, for any triangle
    tri = wr.ladder_rays()[2]
    passes, det, u, v, tt = wr.restate_triangle(o, d, wr.TRIS[tri, 0], wr.TRIS[tri, 1], wr.TRIS[tri, 2])
    out, det0, u0, v0, t0 = wr.restate(o, d, tri)
    assert np.array_equal(passes, out == 0) and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in ((det, det0), (u, u0), (v, v0), (tt, t0)))


def test_the_restated_triangle_test_on_a_shipped_scene(oracle, rpt, world):
    """what the LAST tests decide with (which rays pass an emitter's test; that a record names a triangle the ray passes, at that triangle's t): restate_triangle on
    the triangle the oracle's nearest walk ends on gives the oracle's t and side, bit for bit, on DarkCornell — from the vertices as uploaded, not only on dyadic ones"""
    w = world("DarkCornell")
    o, d, _ = wr._shadow_like_rays(np.random.default_rng(79), 8000, w)
    t_c, tri_c, fl_c, err = oracle.trace_rays(oracle.scene(w), 0, o, d)
    assert err == 0
    hit = (fl_c & 1) == 1
    assert hit.sum() > 4000
    v = w.per_vertex["vertex"][:, :3]
    k = tri_c[hit]
    passes, det, _, _, t = wr.restate_triangle(o[hit], d[hit], v[w.indices["v0"][k]], v[w.indices["v1"][k]], v[w.indices["v2"][k]])
    assert passes.all() and np.array_equal(t.view(np.uint32), t_c[hit].view(np.uint32)) and np.array_equal(np.signbit(det), (fl_c[hit] & 2) == 2)


def test_a_nearly_right_walk_changes_the_answers_of_the_sets(ladder):
    """each near miss against the restatement proper: the (ray, rung) pairs of the shadow sets whose occluded bit changes, and the rays of the nearest sets (the
    ladder's rays and the five fans) whose hit record changes.  Three of the seven are about max_t and can show on shadow rays only."""
    o, d, _, _, t, _, _, rungs = ladder
    nearest = [(o, d)] + [wr.two_leaf_fan(name)[:2] for name in wr.FAN_ORIGINS]
    right_nearest = [wr.walk_two_leaf(no, nd) for no, nd in nearest]
    right_any = {r: wr.walk_two_leaf(o, d, max_t) for r, (max_t, _) in rungs.items()}
    for r, (_, occluded) in rungs.items():
        assert np.array_equal(right_any[r], occluded)
    for miss in wr.NEAR_MISSES:
        shadow = {r: int((wr.walk_two_leaf(o, d, max_t, miss) != right_any[r]).sum()) for r, (max_t, _) in rungs.items()}
        near = []
        for (no, nd), (hit, best, tri, back) in zip(nearest, right_nearest):
            h2, b2, t2, f2 = wr.walk_two_leaf(no, nd, None, miss)
            near.append(int(((h2 != hit) | (b2.view(np.uint32) != best.view(np.uint32)) | (t2 != tri) | (f2 != back)).sum()))
        print(f"{miss}: shadow {sum(shadow.values())} {({r: c for r, c in shadow.items() if c})}, nearest {near}")
        assert sum(shadow.values()) >= ENOUGH, miss
        if miss in ("t < max_t", "NaN max_t accepts", "max_t >= 1e6 bounds"):
            assert sum(near) == 0                                           # (no max_t in a nearest walk)
        else:
            assert near[0] >= ENOUGH, miss                                  # the ladder's rays through the PLAIN and LAST walks
        if miss in ("u + v >= 1 rejected", "back faces rejected"):
            assert min(near[1:]) >= ENOUGH, (miss, near)                    # and every fan through FIRST
    # which rung shows which: on the hit, NaN, and from 1e6 on
    assert (wr.walk_two_leaf(o, d, rungs["t"][0], "t < max_t") != right_any["t"]).sum() >= ENOUGH
    assert (wr.walk_two_leaf(o, d, rungs["nan"][0], "NaN max_t accepts") != right_any["nan"]).sum() >= ENOUGH
    for r in ("2e6", "inf"):
        assert (wr.walk_two_leaf(o, d, rungs[r][0], "max_t >= 1e6 bounds") != right_any[r]).sum() >= ENOUGH


def test_the_segment_model_on_these_sets(sim, oracle, rpt, two_leaf, ladder):  # noqa: F811
    """Recorded, not asserted to be 0: the rays on which the model of the segment rule (sim_any_hit_segment: a box is entered only if also tmin <= max_t) answers
    differently from the model of the exact rule (sim_any_hit_order).  The rule may lose an occlusion where a box's tmin rounds above a triangle's t — which is why
    the production `_seg` kernels are held to the MODEL ray for ray, not to the oracle.  Asserted: the exact model is the oracle, and the rule only ever loses."""
    o, d, _, _, t, _, _, rungs = ladder
    cases = [("two-leaf ladder", two_leaf[1], [(o, d, max_t, occ) for (max_t, occ) in rungs.values()])]
    w = wr.extremes_scene(rpt)
    rng = np.random.default_rng(61)
    eo, ed, em = wr._shadow_like_rays(rng, 8000, w)
    cases.append(("extremes, shadow-like", oracle.scene(w), [(eo, ed, em, None)]))
    for name, sc, sets in cases:
        differ = total = 0
        for so, sd, max_t, occluded in sets:
            n = len(so)
            so, sd, max_t = np.ascontiguousarray(so, F), np.ascontiguousarray(sd, F), np.ascontiguousarray(max_t, F)
            exact, seg = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            sim.sim_any_hit_order(C.byref(sc), C.c_size_t(n), _p(so), _p(sd), _p(max_t), 0, C.c_uint32(0), _p(exact))
            sim.sim_any_hit_segment(C.byref(sc), C.c_size_t(n), _p(so), _p(sd), _p(max_t), 0, C.c_uint32(0), _p(seg))
            if occluded is not None:
                assert np.array_equal(exact == 1, occluded)
            assert not ((seg == 1) & (exact == 0)).any()
            differ += int((seg != exact).sum())
            total += n
        print(f"{name}: the segment model differs from the exact model on {differ} of {total} rays")
