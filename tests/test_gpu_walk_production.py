"""Chosen rays through EVERY walk rpt_render launches, ray by ray (rpt_debug_walk_production: the hook fills the context's slots or its sharded shadow queue and calls
rpt_launch_nearest / rpt_launch_shadow as an iteration does, so the scene, rpt_set_shadow_mode and the developer knobs select the kernel as they do in a render).

  * SHADOW, exact mode: the occluded bit is the oracle's any-hit bit — the streamed LDS walk (near and fixed order) with k_shadow_resolve behind it, the streamed
    global-memory walk for every stack capacity, entry width, leaf build and order, the generic walk of a foreign node pool;
  * SHADOW, segment mode, on the same context: the occluded bit is the bit of the CPU model of the segment rule (tools/anyhit_order_sim.cpp) — the `_seg` twins of
    all of them, held bit for bit — and the exact mode is the oracle's again afterwards;
  * queue shapes from 1 to 4 097 entries in unevenly filled shards: every entry is resolved into its own slot once (the hook checks each radiance record) and the
    shadow-ray counter grows by exactly the number of entries;
  * FIRST (planes staged with the camera's position subtracted): t, triangle and flags are the oracle's from five origins, and another origin is refused;
  * LAST (rays that pass the test of no emitter stop at their first accepted triangle): every order the library knows, three sets of emitters;
  * rays with a NaN or an infinite component, in a test of their own at the end of the file.

The rays are those of tests/walk_rays.py; tests/test_walk_production_rays.py shows without a GPU that they tell the reference's walk from seven nearly right ones."""
import copy
import ctypes as C

import numpy as np
import pytest

import test_gpu_parity as parity
import test_gpu_shadow_segment as segment
import test_gpu_walk_overhead as overhead
import walk_rays as wr
from oracle_ffi import _p
from test_gpu_shadow_segment import sim  # noqa: F401  (the fixture: the CPU models of the exact and the segment rule)

pytestmark = pytest.mark.gpu

F = np.float32
KNOBS = ("RPT_NO_LDS_SCENE", "RPT_COOP_LEAVES", "RPT_STACK_BITS", "RPT_SHADOW_ORDER", "RPT_LAST_ORDER", "RPT_SLOT_Q_SHIFT")
_cache = {}


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _renderer(hipmod, rpt, w, cfg=None, size=(64, 64)):
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        r.set_config(cfg if cfg is not None else rpt.default_config(*size))
        r.reset(rpt.blue_noise_seeds(*size))
    except Exception:
        r.close()
        raise
    return r


def _shadow_refs(key, oracle, sim, sc, o, d, max_t):  # noqa: F811
    """the oracle's any-hit bit and the segment model's bit for a ray set: computed once, never changed"""
    if key not in _cache:
        n = len(o)
        o, d, max_t = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F), np.ascontiguousarray(max_t, F)
        _, _, fl, err = oracle.trace_rays(sc, 1, o, d, max_t)
        assert err == 0
        model = np.zeros(n, np.uint8)
        sim.sim_any_hit_segment(C.byref(sc), C.c_size_t(n), _p(o), _p(d), _p(max_t), 0, C.c_uint32(0), _p(model))
        exact, model = (fl & 1).astype(np.uint32), model.astype(np.uint32)
        exact.setflags(write=False)
        model.setflags(write=False)
        _cache[key] = (exact, model)
    return _cache[key]


def _walk_shadow(r, hipmod, o, d, max_t):
    """one SHADOW call: the occluded bits; the counter grew by the number of rays; t and triangle stay zero"""
    before = r.stats()["shadow_rays"]
    t, tri, flags = r.debug_walk_production(hipmod.WALK_SHADOW, o, d, max_t)
    assert r.stats()["shadow_rays"] - before == len(o)
    assert not t.any() and not tri.any() and not (flags & ~np.uint32(1)).any()
    return flags


def _hold_shadow(r, hipmod, exact, model, o, d, max_t, shapes=wr.QUEUE_SHAPES):
    """exact mode against the oracle, segment mode against the model, exact again, on one context; then every queue shape (a window of the set that begins
    somewhere else for each), in both modes"""
    print(f"{len(o)} rays: {int(exact.sum())} occluded for the oracle, {int(model.sum())} for the segment model ({int((exact != model).sum())} differ)")
    for mode, ref in ((hipmod.SHADOW_EXACT, exact), (hipmod.SHADOW_SEGMENT, model), (hipmod.SHADOW_EXACT, exact)):
        r.set_shadow_mode(mode)
        got = _walk_shadow(r, hipmod, o, d, max_t)
        assert np.array_equal(got, ref), (mode, int((got != ref).sum()), np.flatnonzero(got != ref)[:8])
    for k, n in enumerate(shapes):
        at = (k * 997) % max(1, len(o) - n)
        win = slice(at, at + n)
        for mode, ref in ((hipmod.SHADOW_SEGMENT, model), (hipmod.SHADOW_EXACT, exact)):
            r.set_shadow_mode(mode)
            got = _walk_shadow(r, hipmod, o[win], d[win], max_t[win])
            assert np.array_equal(got, ref[win]), (n, mode, int((got != ref[win]).sum()))


# ---- SHADOW ------------------------------------------------------------------------------------------------------------------------------------------------------

def _ladder(oracle, rpt):
    if "ladder" not in _cache:
        o, d, tri, cls = wr.ladder_rays()
        t, _, fl, err = oracle.trace_rays(oracle.scene(wr.two_leaf_scene(rpt)), 0, o, d)
        assert err == 0
        _cache["ladder"] = (o, d, (fl & 1) == 1, dict(wr.shadow_bounds(t)))
    return _cache["ladder"]


@pytest.mark.parametrize("rungs", [wr.RUNGS[0:5], wr.RUNGS[5:10], wr.RUNGS[10:15]], ids=lambda g: "_".join(g))
def test_shadow_bounds_on_the_two_leaf_scene(monkeypatch, sim, hipmod, oracle, rpt, rungs):  # noqa: F811
    """bound_rays x shadow_bounds through the streamed LDS shadow walk and k_shadow_resolve, and the ladder's known answers"""
    _env(monkeypatch, {})
    w = wr.two_leaf_scene(rpt)
    o1, d1, hit, bounds = _ladder(oracle, rpt)
    o, d, max_t = np.tile(o1, (len(rungs), 1)), np.tile(d1, (len(rungs), 1)), np.concatenate([bounds[g] for g in rungs])
    assert len(o) <= 20_000
    exact, model = _shadow_refs(("two", rungs), oracle, sim, oracle.scene(w), o, d, max_t)
    for k, g in enumerate(rungs):
        occluded = exact[k * len(o1):(k + 1) * len(o1)] == 1
        if g in ("t", "t+", "1e6-") + wr.UNBOUNDED:
            assert np.array_equal(occluded, hit), g                  # t <= max_t holds at max_t == t; from 1e6 on the bound is none
        elif g in ("t-",) + wr.NOTHING:
            assert not occluded.any(), g                             # the hit is its leaf's only candidate: one float nearer it is lost; NaN and bounds <= 0.001 keep nothing
        else:
            assert g == "0.001+" and 32 <= occluded.sum() < hit.sum()
    r = _renderer(hipmod, rpt, w)
    try:
        _hold_shadow(r, hipmod, exact, model, o, d, max_t)
    finally:
        r.close()


def _column_rays(rng, n):
    """the rays of test_full_empty_and_dead_columns_side_by_side (tests/test_gpu_walk_scalar.py): 15 entries high, missing everything, ending early — by lane"""
    o = np.tile(np.array([[0.0, 0.0, -3.0]], F), (n, 1))
    d = np.tile(np.array([[0.0, 0.0, 1.0]], F), (n, 1))
    d[:, :2] += rng.normal(size=(n, 2)).astype(F) * F(0.02)
    away = np.arange(n) % 3 == 1
    d[away] = rng.normal(size=(int(away.sum()), 3)).astype(F) * F([1, 1, 0.2]) + F([0, 0, -1])
    short = np.arange(n) % 3 == 2
    o[short] = np.concatenate([rng.uniform(-4, 4, (int(short.sum()), 2)), rng.uniform(18.2, 18.8, (int(short.sum()), 1))], 1).astype(F)
    return o, d


def _scene_rays(name, w, oracle, sc):
    """(origins, directions, max_t) for a scene of the matrix: shadow-like rays (max_t around the distance to a vertex), and for the small hand-built scenes the
    rays made for them with the part of the ladder that depends on the hit"""
    if ("rays", name) in _cache:
        return _cache[("rays", name)]
    rng = np.random.default_rng(71)
    o, d, max_t = wr._shadow_like_rays(rng, 8000, w)
    if name in ("one_triangle", "extremes"):
        if name == "one_triangle":
            bo, bd, tri, _ = wr.bound_rays()
            bo, bd = bo[tri == 0], bd[tri == 0]
        else:
            bo, bd = _column_rays(rng, 1536)
        t, _, _, err = oracle.trace_rays(sc, 0, bo, bd)
        assert err == 0
        ladder = dict(wr.shadow_bounds(t))
        pick = ("t", "t-", "t+", "inf", "nan", "0.001+")
        o, d = np.concatenate([o] + [bo] * len(pick)), np.concatenate([d] + [bd] * len(pick))
        max_t = np.concatenate([max_t] + [ladder[g] for g in pick])
    assert len(o) <= 20_000
    _cache[("rays", name)] = (o, d, max_t)
    return _cache[("rays", name)]


def _matrix_world(rpt, world, name):
    if name == "one_triangle":
        return wr.one_triangle_scene(rpt)
    if name == "extremes":
        return wr.extremes_scene(rpt)
    return segment._world(world, name)


MATRIX = [("one_triangle", {})]
MATRIX += [(s, {"RPT_SHADOW_ORDER": order}) for s in ("extremes", "DarkCornell") for order in ("near", "fixed")]
MATRIX += [("DarkCornell", {"RPT_NO_LDS_SCENE": "1", "RPT_COOP_LEAVES": coop, "RPT_SHADOW_ORDER": order}) for coop in ("0", "1") for order in ("near", "fixed")]
MATRIX += [("scatter", {"RPT_STACK_BITS": bits, "RPT_COOP_LEAVES": coop, "RPT_SHADOW_ORDER": order}) for bits in ("16", "21", "24", "32") for (coop, order) in (("0", "near"), ("1", "fixed"))]
MATRIX += [("foreign_pool", {})]


@pytest.mark.parametrize("case", MATRIX, ids=lambda c: c[0] + "-" + ("_".join(f"{k[4:].lower()}={v}" for k, v in c[1].items()) or "default"))
def test_shadow_rays_through_every_production_kernel(monkeypatch, sim, hipmod, oracle, rpt, world, case):  # noqa: F811
    name, env = case
    _env(monkeypatch, env)
    w = _matrix_world(rpt, world, name)
    sc = oracle.scene(w)
    o, d, max_t = _scene_rays(name, w, oracle, sc)
    exact, model = _shadow_refs(("matrix", name), oracle, sim, sc, o, d, max_t)
    assert 0.02 * len(o) < exact.sum() < 0.98 * len(o)
    r = _renderer(hipmod, rpt, w)
    try:
        if "RPT_SHADOW_ORDER" in env:
            so = r.shadow_order()                                     # (a scene on which no probe ray can be formed — the extremes scene — keeps the near order whatever is asked)
            print(f"{name}: fixed order {so['fixed']}, {so['probe_rays']} probe rays")
            assert so["fixed"] == (env["RPT_SHADOW_ORDER"] == "fixed" and so["probe_rays"] > 0)
            assert so["probe_rays"] > 0 or name == "extremes"
        _hold_shadow(r, hipmod, exact, model, o, d, max_t, shapes=(1, 15, 65, 257))
    finally:
        r.close()


def test_what_the_hook_refuses(hipmod, rpt):
    w = wr.two_leaf_scene(rpt)
    o, d = wr.ladder_rays()[:2]
    r = hipmod.Renderer(0)
    try:
        def refused(*args):
            with pytest.raises(hipmod.RptError) as e:
                r.debug_walk_production(*args)
            assert e.value.code == -1, e.value
        refused(hipmod.WALK_SHADOW, o[:4], d[:4], np.ones(4, F))                                   # no scene
        r.upload_scene(w)
        refused(hipmod.WALK_NEAREST_PLAIN, o[:4], d[:4])                                           # no configuration
        r.set_config(rpt.default_config(8, 8))
        r.reset(rpt.blue_noise_seeds(8, 8))
        refused(hipmod.WALK_SHADOW, o[:4], d[:4])                                                  # shadow rays without max_t
        refused(4, o[:4], d[:4])
        for kind in (hipmod.WALK_NEAREST_PLAIN, hipmod.WALK_NEAREST_LAST, hipmod.WALK_SHADOW):
            t, tri, fl = r.debug_walk_production(kind, o[:0], d[:0], np.ones(0, F))                # no rays: nothing launched
            assert len(t) == len(tri) == len(fl) == 0
        slots = 64 * 32                                                                            # 8 x 8 pixels padded to a chunk, at most 32 samples of each in flight
        many = np.resize(np.arange(len(o)), slots + 1)
        for kind in (hipmod.WALK_NEAREST_PLAIN, hipmod.WALK_SHADOW):
            refused(kind, o[many], d[many], np.ones(len(many), F))                                 # more rays than slots
        t, tri, fl = r.debug_walk_production(hipmod.WALK_NEAREST_PLAIN, o[many[:slots]], d[many[:slots]])
        assert (fl & 1).sum() > 100
    finally:
        r.close()


# ---- FIRST -------------------------------------------------------------------------------------------------------------------------------------------------------

def _hold_nearest(r, kind, oracle, sc, o, d):
    t_c, tri_c, fl_c, err = oracle.trace_rays(sc, 0, o, d)
    assert err == 0
    hit = (fl_c & 1) == 1
    t_g, tri_g, fl_g = r.debug_walk_production(kind, o, d)
    assert np.array_equal(fl_g, fl_c), int((fl_g != fl_c).sum())
    assert np.array_equal(t_g.view(np.uint32), t_c.view(np.uint32)) and np.array_equal(tri_g[hit], tri_c[hit])
    return hit


@pytest.mark.parametrize("q_shift", [None, "3"])
@pytest.mark.parametrize("scene", ["two_leaf", "extremes", "DarkCornell"])
def test_first_walk_from_one_origin(monkeypatch, hipmod, oracle, rpt, world, scene, q_shift):
    """k_traverse_nearest_stream<.., FIRST>: every ray from cfg.cam_position.  The two-leaf scene from the five origins of walk_rays.fan; the extremes scene with rays
    15 entries high beside rays that miss everything; DarkCornell towards its vertices and between them."""
    _env(monkeypatch, {} if q_shift is None else {"RPT_SLOT_Q_SHIFT": q_shift})
    if scene == "two_leaf":
        w = wr.two_leaf_scene(rpt)
        fans = [wr.two_leaf_fan(name)[:2] for name in wr.FAN_ORIGINS]
    elif scene == "extremes":
        w = wr.extremes_scene(rpt)
        origin = np.array(overhead.EXTREME_VIEW["cam_position"][:3], F)
        d = _column_rays(np.random.default_rng(73), 3072)[1]
        d[2::3] = d[0::3] * F([-1, 1, 1]) + F([0.3, 0, 0])                 # (the third kind there starts elsewhere; here: aside of the axis)
        fans = [(np.tile(origin, (len(d), 1)), d)]
    else:
        w = world("DarkCornell")
        origin = np.array(list(rpt.default_config(64, 64).cam_position)[:3], F)
        v = w.per_vertex["vertex"][:, :3]
        fans = [wr.fan(origin, v[np.random.default_rng(74).integers(0, len(v), 1500)], n_random=1500)]
    assert sum(len(f[0]) for f in fans) <= 20_000
    sc = oracle.scene(w)
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        for o, d in fans:
            r.set_config(rpt.default_config(64, 64, cam_position=(float(o[0, 0]), float(o[0, 1]), float(o[0, 2]), 0.0)))
            r.reset(rpt.blue_noise_seeds(64, 64))
            hit = _hold_nearest(r, hipmod.WALK_NEAREST_FIRST, oracle, sc, o, d)
            assert 32 <= hit.sum() <= len(o) - 32
            # an origin that differs from cam_position in one bit is refused, wherever in the set it stands
            other = o.copy()
            other[len(o) // 2, 1] = np.nextafter(other[len(o) // 2, 1], F(np.inf))
            with pytest.raises(hipmod.RptError) as e:
                r.debug_walk_production(hipmod.WALK_NEAREST_FIRST, other, d)
            assert e.value.code == -1 and "cam_position" in str(e.value)
            _hold_nearest(r, hipmod.WALK_NEAREST_PLAIN, oracle, sc, other, d)        # (the PLAIN walk takes any origin)
    finally:
        r.close()


# ---- LAST --------------------------------------------------------------------------------------------------------------------------------------------------------

def _last_scene(rpt, world, name):
    if ("last", name) in _cache:
        return _cache[("last", name)]
    if name == "two_leaf_T1_emits":
        w = copy.copy(wr.two_leaf_scene(rpt))
        w.materials = w.materials.copy()
        w.materials["emissive"][:] = 0
        w.materials["emissive"][1] = (1.5, 0.25, 4.0, 0.0)                   # T1's material, and only it
        o, d = wr.ladder_rays()[:2]
        fo, fd = wr.two_leaf_fan("outside")[:2]
        o, d = np.concatenate([o, fo]), np.concatenate([d, fd])
    else:
        w, n_em = parity._with_emissive_materials(rpt, world("DarkCornell"), 4 if name == "four_emitters" else 40)
        assert (2 < n_em <= 4) if name == "four_emitters" else n_em > 4
        rng = np.random.default_rng(79)
        o, d, _ = wr._shadow_like_rays(rng, 8000, w)
        # a quarter of the rays towards the emitters
        em = _emissive_triangles(w)
        v = w.per_vertex["vertex"][:, :3]
        tr = w.indices[em[rng.integers(0, len(em), 2000)]]
        bary = rng.dirichlet((1.0, 1.0, 1.0), 2000)
        target = bary[:, :1] * v[tr["v0"]] + bary[:, 1:2] * v[tr["v1"]] + bary[:, 2:] * v[tr["v2"]]
        d[:2000] = (target - o[:2000]) / np.linalg.norm(target - o[:2000], axis=1, keepdims=True)
        d[d == 0] = F(2.0 ** -20)
    _cache[("last", name)] = (w, np.ascontiguousarray(o, F), np.ascontiguousarray(d, F))
    return _cache[("last", name)]


def _emissive_triangles(w):
    em = w.materials["emissive"][:, :3]
    return np.flatnonzero(np.any(em[w.indices["material"]] != 0, axis=1))


def _hold_last(r, hipmod, oracle, w, o, d, stops_early):
    """one LAST call held to the oracle as far as the launch promises (test_last_walk_ray_by_ray); returns (hit, passes an emitter's test, may have stopped early)"""
    t_c, tri_c, fl_c, err = oracle.trace_rays(oracle.scene(w), 0, o, d)
    assert err == 0
    v = w.per_vertex["vertex"][:, :3]
    corners = lambda k: (v[w.indices["v0"][k]], v[w.indices["v1"][k]], v[w.indices["v2"][k]])
    em = _emissive_triangles(w)
    may_emit = np.zeros(len(o), bool)
    for k in em[:8]:                                                          # (more than four: the plain launch, every record is the oracle's anyway)
        may_emit |= wr.restate_triangle(o, d, *corners(k))[0]
    t_g, tri_g, fl_g = r.debug_walk_production(hipmod.WALK_NEAREST_LAST, o, d)
    hit = (fl_c & 1) == 1
    assert np.array_equal(fl_g & 1, fl_c & 1), int(((fl_g ^ fl_c) & 1).sum())
    whole = may_emit if stops_early else np.ones(len(o), bool)
    assert np.array_equal(fl_g[whole], fl_c[whole]) and np.array_equal(t_g[whole].view(np.uint32), t_c[whole].view(np.uint32))
    assert np.array_equal(tri_g[whole & hit], tri_c[whole & hit])
    rest = hit & ~whole
    print(f"{int(hit.sum())} of {len(o)} rays hit; {int((whole & hit).sum())} walked to the end, {int(rest.sum())} may have stopped at their first hit, "
          f"{int((tri_g[rest] != tri_c[rest]).sum())} of them on another triangle than the nearest")
    if rest.any():
        k = tri_g[rest]
        assert k.max() < len(w.indices) and not np.isin(k, em).any()
        passes, det, _, _, t_own = wr.restate_triangle(o[rest], d[rest], *corners(k))
        assert passes.all() and np.array_equal(t_g[rest].view(np.uint32), t_own.view(np.uint32))
        assert np.array_equal((fl_g[rest] & 2) == 2, np.signbit(det))
        assert np.all(t_own > wr.EPS) and np.all(t_own >= t_c[rest])          # accepted (t > 0.001), and not nearer than the nearest
    return hit, may_emit, rest


@pytest.mark.parametrize("mode", sorted(parity.LAST_MODES))
@pytest.mark.parametrize("scene", ["two_leaf_T1_emits", "four_emitters", "too_many_emitters"])
def test_last_walk_ray_by_ray(monkeypatch, hipmod, oracle, rpt, world, scene, mode):
    """k_traverse_nearest_stream<.., LAST> in the form that writes hit records.  Hit or miss is the oracle's for every ray; a ray that passes the Moller-Trumbore
    test of an emissive triangle (walk_rays.restate_triangle, float32 numpy) walked to the end: the oracle's whole record; any other ray that hit may have stopped
    at its first accepted triangle: the record names a triangle whose test the ray passes, which does not emit, with that triangle's t and side."""
    var, val, expect = parity.LAST_MODES[mode]
    _env(monkeypatch, {var: val})
    w, o, d = _last_scene(rpt, world, scene)
    assert len(o) <= 20_000
    r = _renderer(hipmod, rpt, w)
    try:
        lo = r.last_bounce_order()
        print(f"{scene}, {mode}: {lo['mode_is']}, {lo['probe_rays']} probe rays")
        if scene == "too_many_emitters" or expect == 0:
            assert lo["mode"] == 0, lo
        else:                                                                 # (a scene on which no probe ray can be formed keeps the near order whatever is asked)
            assert lo["mode"] == (expect if lo["probe_rays"] > 0 else 1), lo
        hit, may_emit, rest = _hold_last(r, hipmod, oracle, w, o, d, lo["mode"] != 0)
    finally:
        r.close()
    assert (may_emit & hit).sum() >= 32 and (~may_emit & hit).sum() >= 32 and (~hit).sum() >= 32
    assert (rest.sum() >= 32) == (lo["mode"] != 0)


# ---- NaN and infinity: last in the file ----------------------------------------------------------------------------------------------------------------------------

def test_rays_with_a_nan_or_an_infinite_component(sim, hipmod, oracle, rpt):  # noqa: F811
    """special_rays (one component of the origin or the direction NaN or +-inf) through SHADOW in both modes under finite, NaN and infinite bounds, and through LAST;
    the same directions from the camera's position through FIRST.  Every answer is the oracle's (segment mode: the model's), and the context renders the oracle's image
    afterwards, as after the PLAIN production walk (tests/test_gpu_parity.py test_ray_parity_through_the_production_traversal_stage)."""
    w = wr.two_leaf_scene(rpt)
    sc = oracle.scene(w)
    so, sd = wr.special_rays()
    bounds = [np.full(len(so), b, F) for b in (2.0, 2.0e6, np.inf, -np.inf, np.nan)]
    o, d, max_t = np.tile(so, (len(bounds), 1)), np.tile(sd, (len(bounds), 1)), np.concatenate(bounds)
    exact, model = _shadow_refs("special", oracle, sim, sc, o, d, max_t)
    cam = np.array([1.1, 0.3, -3.2], F)
    fo, fd = np.tile(cam, (len(sd), 1)), sd.copy()
    cfg = rpt.default_config(64, 48, cam_position=(float(cam[0]), float(cam[1]), float(cam[2]), 0.0))
    seeds = rpt.blue_noise_seeds(64, 48)
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        r.set_config(cfg)
        r.reset(seeds)
        _hold_shadow(r, hipmod, exact, model, o, d, max_t, shapes=(15, 65))
        _hold_last(r, hipmod, oracle, w, so, sd, r.last_bounce_order()["mode"] != 0)
        _hold_nearest(r, hipmod.WALK_NEAREST_FIRST, oracle, sc, fo, fd)
        r.reset(seeds)
        r.render(1)
        acc, _ = r.read_accum()
    finally:
        r.close()
    ref, _, _ = oracle.trace_cpu(cfg, sc, seeds, 1)
    assert np.array_equal(acc.view(np.uint32), ref.view(np.uint32))
