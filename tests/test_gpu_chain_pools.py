"""The walks at the limits of the node pools rpt_upload_scene accepts (tests/chain_pools.py; tests/test_chain_pools.py shows without a GPU what each pool is and that
its rays tell the device's stack discipline from the nearly right ones).  Every case drives Renderer.debug_walk_production and holds each kind to the oracle bit for
bit on t, triangle and flags — WALK_NEAREST_PLAIN, WALK_NEAREST_LAST, and WALK_SHADOW in exact mode, then segment mode (held to the CPU model of the segment rule),
then exact again — then the debug kernels (nearest, any hit, segment) on the same rays, and ends with one 64 x 64, 2-spp, nee 1 render from (0, 0, -3) whose
accumulators, rng and ray counts are the oracle's.

  pool                                   environment                                      kernels it reaches
  compact15                              RPT_NO_LDS_SCENE=1; RPT_SHADOW_ORDER near, fixed  gstream <16, 16>, 15 of 16 entries
  compact16, compact23                   RPT_STACK_BITS unset, 21, 24                      gstream <24, 16 / 21 / 24>, either side of the 16 -> 24 step, 23 of 24 entries
  compact24, compact31                   RPT_STACK_BITS unset, 21, 24, 32                  gstream <32, *>, 31 of 32 entries
  compact24fat, compact31fat             RPT_COOP_LEAVES 0, 1                              the same with one leaf of 63 triangles, either leaf build
  foreign31                              -                                                 the generic k_traverse_nearest<32>, k_traverse_shadow<32> and _seg
  sparse15_65535                         -                                                 16-bit entries at their largest, 65 533 / 65 534
  sparse15_65565                         -                                                 a tree of 15 levels with links from 65 536 on: 24 entries of 21 bits
  sparse16_2m-, sparse31_2m-             -                                                 21-bit entries, all five mask bits, a stale mask bit cleared
  sparse16_2m+, sparse31_2m+             -                                                 24-bit entries (Stack24) in the 24- and the 32-entry stack
  right_child_2^24                       -                                                 not pair-shaped (asserted BEFORE a ray is walked): the generic walks

Before the rays each case asserts what the context reports about the pool — whether it is pair-shaped and how many probe rays were walked (shadow_order(); the host
build of the probe says the same), the order asked for, that no LDS walk is in play — and that between 32 and n - 32 rays hit."""
import time

import numpy as np
import pytest

import chain_pools as cp
import test_gpu_walk_production as prod
from test_gpu_shadow_segment import sim  # noqa: F401  (the fixture: the CPU models of the exact and the segment rule)

pytestmark = pytest.mark.gpu

F = np.float32
NOT_PAIR_SHAPED = "node pool is not pair-shaped"
_cache = {}

CASES = [("compact15", {"RPT_NO_LDS_SCENE": "1", "RPT_SHADOW_ORDER": order}) for order in ("near", "fixed")]
CASES += [(p, {} if bits is None else {"RPT_STACK_BITS": bits}) for p in ("compact16", "compact23") for bits in (None, "21", "24")]
CASES += [(p, {} if bits is None else {"RPT_STACK_BITS": bits}) for p in ("compact24", "compact31") for bits in (None, "21", "24", "32")]
CASES += [(p, {"RPT_COOP_LEAVES": coop}) for p in ("compact24fat", "compact31fat") for coop in ("0", "1")]
CASES += [(p, {}) for p in ("foreign31", "sparse15_65535", "sparse15_65565") + cp.LARGE_POOLS]


def _refs(oracle, sim, rpt, name, segment=True):  # noqa: F811
    """everything the oracle (and the segment model) says about a pool: computed once, never changed"""
    if name in _cache:
        return _cache[name]
    w = cp.pool(rpt, name)
    sc = oracle.scene(w)
    o, d = cp.nearest_rays()
    t, tri, fl, err = oracle.trace_rays(sc, 0, o, d)
    assert err == 0
    so, sd, max_t = cp.shadow_rays(lambda oo, dd: oracle.trace_rays(sc, 0, oo, dd)[0])
    assert len(o) <= 8192 and len(so) <= 8192
    if segment:
        exact, model = prod._shadow_refs(("chain", name), oracle, sim, sc, so, sd, max_t)
    else:
        _, _, afl, err = oracle.trace_rays(sc, 1, so, sd, max_t)
        assert err == 0
        exact, model = (afl & 1).astype(np.uint32), None
    cfg = rpt.default_config(64, 64, nee=1, **cp.VIEW)
    seeds = rpt.blue_noise_seeds(64, 64)
    acc, rng, st = oracle.trace_cpu(cfg, sc, seeds, 2)
    assert st.error_flags == 0
    for a in (t, tri, fl, acc, rng):
        a.setflags(write=False)
    _cache[name] = dict(w=w, sc=sc, o=o, d=d, t=t, tri=tri, fl=fl, so=so, sd=sd, max_t=max_t, exact=exact, model=model, cfg=cfg, seeds=seeds, acc=acc, rng=rng, st=st)
    return _cache[name]


def _hold_render(r, ref):
    """after the hook: reset, then 2 samples per pixel — accumulators, rng and ray counts are the oracle's"""
    r.reset(ref["seeds"])
    before = r.stats()
    r.render(2)
    acc, samples = r.read_accum()
    st, st_c = r.stats(), ref["st"]
    assert samples == 2
    assert st["extension_rays"] - before["extension_rays"] == st_c.extension_rays and st["shadow_rays"] - before["shadow_rays"] == st_c.shadow_rays
    assert st["sky_evals"] - before["sky_evals"] == st_c.sky_evals
    differ = acc.view(np.uint32) != ref["acc"].view(np.uint32)
    assert not differ.any(), f"{int(differ.sum())} accumulator words differ"
    assert np.array_equal(r.read_rng().reshape(-1), np.asarray(ref["rng"]).reshape(-1))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0] + "-" + ("_".join(f"{k[4:].lower()}={v}" for k, v in c[1].items()) or "default"))
def test_the_walks_at_the_limits_of_a_pool(monkeypatch, sim, hipmod, oracle, rpt, case):  # noqa: F811
    name, env = case
    prod._env(monkeypatch, env)
    ref = _refs(oracle, sim, rpt, name)
    w, sc, o, d = ref["w"], ref["sc"], ref["o"], ref["d"]
    hit = (ref["fl"] & 1) == 1
    assert 32 <= hit.sum() <= len(o) - 32 and 32 <= ref["exact"].sum() <= len(ref["so"]) - 32
    host = hipmod.shadow_order_host(w)                                  # (reads RPT_SHADOW_ORDER as the upload does)
    t0 = time.perf_counter()
    r = prod._renderer(hipmod, rpt, w, cfg=ref["cfg"])
    try:
        # what the context says about the pool
        so, lo = r.shadow_order(), r.last_bounce_order()
        print(f"{name} {env}: {so['why']}; fixed order {so['fixed']}, {so['probe_rays']} probe rays; last rays: {lo['mode_is']}")
        pair_shaped = name != "foreign31"
        assert (so["why"] != NOT_PAIR_SHAPED) == pair_shaped and (host["why"] != NOT_PAIR_SHAPED) == pair_shaped
        assert so["probe_rays"] == host["probe_rays"] and (so["probe_rays"] > 0) == pair_shaped
        assert so["fixed"] == (env["RPT_SHADOW_ORDER"] == "fixed" if "RPT_SHADOW_ORDER" in env else host["fixed"])
        assert lo["mode"] == 0                                          # no LDS image in play (RPT_NO_LDS_SCENE, or a pool no image takes): the global-memory walks
        # the production walks
        got = prod._hold_nearest(r, hipmod.WALK_NEAREST_PLAIN, oracle, sc, o, d)
        assert np.array_equal(got, hit)
        prod._hold_last(r, hipmod, oracle, w, o, d, False)
        prod._hold_shadow(r, hipmod, ref["exact"], ref["model"], ref["so"], ref["sd"], ref["max_t"], shapes=(1, 65))
        # the debug kernels on the same rays
        t_g, tri_g, fl_g = r.debug_trace_rays(0, o, d)
        assert np.array_equal(fl_g, ref["fl"]) and np.array_equal(t_g.view(np.uint32), ref["t"].view(np.uint32)) and np.array_equal(tri_g[hit], ref["tri"][hit])
        for kind, want in ((1, ref["exact"]), (2, ref["model"])):
            _, _, afl = r.debug_trace_rays(kind, ref["so"], ref["sd"], ref["max_t"])
            assert np.array_equal(afl & 1, want), (kind, int(((afl & 1) != want).sum()))
        _hold_render(r, ref)
    finally:
        r.close()
    print(f"{name}: {time.perf_counter() - t0:.2f} s on the device side of the case")


def test_a_right_child_at_node_2_to_the_24_keeps_the_generic_walks(monkeypatch, sim, hipmod, oracle, rpt):  # noqa: F811
    """A tree of 16 levels in a pool of 2^24 + 1 nodes (512 MB) whose second inner node has left_or_first = 2^24 - 1: its right child is node 2^24, which the 24-bit
    entries of a 24-entry stack would bring back as node 0.  The context must report the pool as NOT pair-shaped — asserted before any ray is walked — and then
    4 096 rays through WALK_NEAREST_PLAIN and shadow rays through WALK_SHADOW are the oracle's."""
    prod._env(monkeypatch, {})
    name = "right_child_2^24"
    w = cp.pool(rpt, name)
    assert len(w.nodes) == (1 << 24) + 1 and cp.tree_facts(w.nodes)[0] == 16 and ((1 << 24) - 1) in w.nodes["left_or_first"][w.nodes["triangle_count"] == 0]
    sc = oracle.scene(w)
    o, d = cp.bundle(cp.BACK_Z)                                          # from z = +60: the rays that push the right child
    so_, sd_, max_t = cp.shadow_rays(lambda oo, dd: oracle.trace_rays(sc, 0, oo, dd)[0])
    t0 = time.perf_counter()
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        upload_s = time.perf_counter() - t0
        print(f"upload of the 2^24 + 1 nodes: {upload_s:.2f} s")
        so = r.shadow_order()
        assert so["why"] == NOT_PAIR_SHAPED and so["probe_rays"] == 0 and not so["fixed"], so
        # only now the rays
        r.set_config(rpt.default_config(64, 64))
        r.reset(rpt.blue_noise_seeds(64, 64))
        hit = prod._hold_nearest(r, hipmod.WALK_NEAREST_PLAIN, oracle, sc, o, d)
        assert 32 <= hit.sum() <= len(o) - 32
        _, _, afl, err = oracle.trace_rays(sc, 1, so_, sd_, max_t)
        assert err == 0 and 32 <= (afl & 1).sum() <= len(so_) - 32
        got = prod._walk_shadow(r, hipmod, so_, sd_, max_t)
        assert np.array_equal(got, afl & 1), int((got != (afl & 1)).sum())
    finally:
        r.close()
    print(f"the case: {time.perf_counter() - t0:.2f} s")
