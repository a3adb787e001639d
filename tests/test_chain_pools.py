"""The node pools of tests/chain_pools.py, without a GPU: that each pool is what tests/test_gpu_chain_pools.py takes it for, that the oracle's walk over them is right
(a brute force over all triangles in float64), and that the rays tell the device's stack discipline from six nearly right ones (chain_pools.walk_model, in the
manner of tests/test_walk_production_rays.py: the CPU tests count the answers a planted fault changes, in the place of planting wrong kernels on a GPU).

  pool                     nodes        depth  what it is for
  compact15                31           15     the 16-entry stack of the global-memory walks at its 15 entries (RPT_NO_LDS_SCENE)
  compact16, compact23     33, 47       16, 23 the 24-entry stack on either side of the 16 -> 24 step, and at 23 entries
  compact24, compact31     49, 63       24, 31 the 32-entry stack, at 31 entries; `fat`: one leaf of 63 triangles (RPT_COOP_LEAVES)
  foreign31                64           31     pairs at (even, odd): the generic walks
  sparse15_65535           65 535       15     16-bit entries at their largest: 65 533 and 65 534 are pushed
  sparse15_65565           65 565       15     a shallow tree with links from 65 536 on: it must NOT get 16-bit entries
  sparse16_2m-, 31_2m-     2^21 - 1     16, 31 21-bit entries with all five mask bits set (up to 2^21 - 2); one level written high then low, another low then high
  sparse16_2m+, 31_2m+     2^21 + 33    16, 31 24-bit entries (from 2^21 + 1 on) in the 24- and the 32-entry stack; the same two levels
  compact32                65           32     one level too deep: refused
  right_child_2^24         2^24 + 1     16     an inner node whose right child is node 2^24: not pair-shaped

Figures (this module prints them; 8 192 rays per pool): the rays left out of the comparison with the brute force because they pass within 1e-4 (in barycentrics) of
an edge are 0.48 % to 1.07 % of a pool's rays (cap 2 %); the largest relative difference between the oracle's t and the float64 t over all pools is 1.06e-7, the
tolerance eight times that, 8.5e-7."""
import numpy as np
import pytest

import chain_pools as cp

FLAGGED_CAP = 0.02                  # a cap, not a measurement
T_MEASURED = 1.06e-7                # largest |t - t64| / t64 over all pools, as printed by test_the_oracle_against_brute_force
T_TOLERANCE = 8 * T_MEASURED
_cache = {}

EXPECT = {  # name: (nodes, depth)
    "compact15": (31, 15), "compact16": (33, 16), "compact23": (47, 23), "compact24": (49, 24), "compact31": (63, 31), "compact24fat": (49, 24),
    "compact31fat": (63, 31), "foreign31": (64, 31), "sparse15_65535": (65535, 15), "sparse15_65565": (65565, 15),
    "sparse16_2m-": ((1 << 21) - 1, 16), "sparse31_2m-": ((1 << 21) - 1, 31), "sparse16_2m+": ((1 << 21) + 33, 16), "sparse31_2m+": ((1 << 21) + 33, 31),
}


def _oracle_rays(oracle, rpt, name):
    """the oracle's nearest hits of chain_pools.nearest_rays over a pool: computed once, never changed"""
    if name not in _cache:
        w = cp.pool(rpt, name)
        o, d = cp.nearest_rays()
        t, tri, fl, err = oracle.trace_rays(oracle.scene(w), 0, o, d)
        assert err == 0
        for a in (t, tri, fl):
            a.setflags(write=False)
        _cache[name] = (t, tri, fl)
    return _cache[name]


@pytest.mark.parametrize("name", cp.POOLS)
def test_the_pools_are_what_they_say(oracle, rpt, name):
    w = cp.pool(rpt, name)
    nodes = w.nodes
    depth, reach = cp.tree_facts(nodes)
    assert (len(nodes), depth) == EXPECT[name] and w.bvh_max_depth == depth
    n_layers = depth + 1
    twice = cp.levels_written_twice(nodes)
    assert len(reach) == 2 * n_layers - 1 + 2 * len(twice)
    inner = [i for i in reach if nodes["triangle_count"][i] == 0]
    # pair-shaped (or, the foreign pool, every pair at an even index), leaves of fewer than 255 triangles
    assert all(int(nodes["left_or_first"][i]) % 2 == (0 if name == "foreign31" else 1) for i in inner)
    assert len(nodes) % 2 == (0 if name == "foreign31" else 1) and nodes["triangle_count"].max() == (63 if name.endswith("fat") else 1)
    # nothing but the tree is an inner node: a wrong index leads to a leaf
    assert int((nodes["triangle_count"] == 0).sum()) == len(inner)
    assert cp.residue_unsafe(nodes) == []
    pushed = [int(nodes["left_or_first"][i]) + s for i in inner for s in (0, 1)]
    if name == "sparse15_65535":
        assert 65533 in pushed and 65534 in pushed and max(pushed) == 65534
    if name == "sparse15_65565":
        assert max(pushed) == 65564 and sum(p >= 65536 for p in pushed) == 28 and 65536 not in reach
    if name.endswith("2m-"):
        assert max(pushed) == (1 << 21) - 2 and (1 << 21) - 3 in pushed                       # 0x1ffffd: all five mask bits and the word's upper bits
    if name.endswith("2m+"):
        assert max(pushed) == (1 << 21) + 32 and sum(p > (1 << 21) for p in pushed) >= 16 and (1 << 21) not in reach
    if name.startswith("sparse") and name != "sparse15_65565":
        # one level written first with an entry whose bits from 16 on are set and then with one in which they are clear, another level the other way round
        # (in the 65 535-node pool: the word's upper bits)
        top = 8 if name == "sparse15_65535" else 16
        kinds = {(a >> top != 0, b >> top != 0) for _, a, b in twice}
        assert kinds == {(True, False), (False, True)}, twice
    # a ray along the axis is inside every box in x and y: both children are hit at every inner node of the chain
    chain = [i for i in inner if reach[i] == 0 or i % 2 == (1 if name == "foreign31" else 0)]
    assert len(chain) == depth
    for i in chain:
        for c in (int(nodes["left_or_first"][i]), int(nodes["left_or_first"][i]) + 1):
            assert (nodes["aabb_min"][c][:2] < -0.1).all() and (nodes["aabb_max"][c][:2] > 0.1).all()
    # the oracle's stack holds the near child too: depth + 1 entries
    cfg = rpt.default_config(64, 64, nee=1, **cp.VIEW)
    _, _, st = oracle.trace_cpu(cfg, oracle.scene(w), rpt.blue_noise_seeds(64, 64), 2)
    assert st.max_stack == depth + 1 and st.error_flags == 0


def test_one_level_more_overflows_the_reference_stack(hipmod, oracle, rpt):
    w = cp.pool(rpt, "compact32")
    assert cp.tree_facts(w.nodes)[0] == 32 and len(w.nodes) == 65
    cfg = rpt.default_config(64, 64, nee=1, **cp.VIEW)
    _, _, st = oracle.trace_cpu(cfg, oracle.scene(w), rpt.blue_noise_seeds(64, 64), 2)
    assert st.error_flags & 1
    with pytest.raises(hipmod.RptError) as e:                           # (the host probes validate as rpt_upload_scene does)
        hipmod.shadow_order_host(w)
    assert e.value.code == -5


@pytest.mark.parametrize("name", cp.POOLS)
def test_the_oracle_against_brute_force(oracle, rpt, name):
    """Hit or miss and the triangle are those of Moller-Trumbore over ALL triangles in float64 for every ray that passes no edge within 1e-4 in barycentrics — at most
    2 % of a pool's rays may be left out that way (measured: 0.48 % to 1.07 %) — and t is the float64 t within 8.5e-7, eight times the largest difference measured
    over all pools (1.06e-7)."""
    w = cp.pool(rpt, name)
    o, d = cp.nearest_rays()
    t, tri, fl = _oracle_rays(oracle, rpt, name)
    hit = (fl & 1) == 1
    bh, bt, btri, edge = cp.brute_force(w, o, d)
    clear = edge >= 1e-4
    rel = np.abs(t[hit & clear].astype(np.float64) - bt[hit & clear]) / bt[hit & clear]
    print(f"{name}: {(~clear).mean() * 100:.2f} % of the rays within 1e-4 of an edge; largest |t - t64| / t64 = {rel.max():.3e}")
    assert (~clear).mean() <= FLAGGED_CAP
    assert np.array_equal(bh[clear], hit[clear]) and np.array_equal(btri[clear & hit], tri[clear & hit] & 0x7fffffff)
    assert rel.max() <= T_TOLERANCE
    for part in (slice(0, len(o) // 2), slice(len(o) // 2, None)):                            # from z = -3, from z = +60
        assert 32 <= hit[part].sum() <= len(o) // 2 - 32


def _differs(model, ref):
    """rays whose answer a model changes: hit or miss, t to the bit, the triangle"""
    mh, mt, mtri, mback, _ = model
    t, tri, fl = ref
    hit = (fl & 1) == 1
    return (mh != hit) | (mt.view(np.uint32) != t.view(np.uint32)) | (hit & mh & ((mtri != tri) | (mback != ((fl & 2) == 2))))


@pytest.mark.parametrize("name", cp.POOLS)
def test_the_model_with_the_librarys_choice_is_the_oracle(oracle, rpt, name):
    w = cp.pool(rpt, name)
    o, d = cp.nearest_rays()
    cap, bits = cp.library_choice(w)
    depth = EXPECT[name][1]
    assert cap == (32 if name == "foreign31" else 16 if name in ("compact15", "sparse15_65535") else 24 if depth <= 23 else 32)
    assert bits == (32 if name == "foreign31" else 16 if len(w.nodes) < 65536 else 21 if len(w.nodes) < (1 << 21) else 24)
    model = cp.walk_model(w, o, d, bits, cap)
    assert model[4].all() and not _differs(model, _oracle_rays(oracle, rpt, name)).any()


FAULTS = [  # (what, pool, entry bits, capacity, clears stale bits)
    ("16-bit entries in the 65 565-node pool of 15 levels", "sparse15_65565", 16, 16, True),
    ("21-bit entries with links from 2^21 on, 24 entries", "sparse16_2m+", 21, 24, True),
    ("21-bit entries with links from 2^21 on, 32 entries", "sparse31_2m+", 21, 32, True),
    ("24-bit entries with a right child at 2^24", "right_child_2^24", 24, 24, True),
    ("15 entries at depth 16", "compact16", 16, 15, True),
    ("23 entries at depth 24", "compact24", 16, 23, True),
    ("mask bits set and never cleared, 24 entries", "sparse16_2m-", 21, 24, False),
    ("mask bits set and never cleared, 32 entries", "sparse31_2m-", 21, 32, False),
]


@pytest.mark.parametrize("fault", FAULTS, ids=lambda f: f[0])
def test_a_planted_fault_changes_answers(oracle, rpt, fault):
    """Each nearly right stack changes at least 32 answers or leaves at least 32 rays walking at the step limit.  (A walk that keeps the near child in hand needs as
    many entries as the tree has levels under the root, so 16 entries still hold a tree of depth 16 and 24 one of depth 24 — asserted below; the library's
    capacities leave one entry over, and the faults planted here are the capacities one BELOW the depth.)"""
    what, name, bits, cap, clears = fault
    w = cp.pool(rpt, name)
    o, d = cp.nearest_rays()
    ref = _oracle_rays(oracle, rpt, name)
    model = cp.walk_model(w, o, d, bits, cap, clears_stale_bits=clears, step_limit=512)
    changed, walking = _differs(model, ref), ~model[4]
    print(f"{what}: {int(changed.sum())} answers changed ({int(changed[:4096].sum())} from z = -3, {int(changed[4096:].sum())} from z = +60), "
          f"{int(walking.sum())} rays unfinished after 512 steps")
    assert changed.sum() >= 32 or walking.sum() >= 32
    if name == "right_child_2^24":
        assert walking.sum() >= 32                                      # entry 2^24 comes back as node 0: the walk starts over, for ever
        whole = cp.walk_model(w, o, d, 32, 32)
        assert whole[4].all() and not _differs(whole, ref).any()
    if not clears:
        assert changed[:4096].sum() >= 32 and changed[4096:].sum() >= 32  # the twins (rays from z = -3), and level 0 written again and again (rays from z = +60)
    if name.startswith("compact"):
        depth = EXPECT[name][1]
        enough = cp.walk_model(w, o, d, bits, depth)
        assert cap == depth - 1 and enough[4].all() and not _differs(enough, ref).any()


def test_the_host_twin_of_the_pair_shape_rule(hipmod, rpt):
    """rpt_scene.hip pool_is_pair_shaped(nodes, nn) behind rpt_debug_shadow_order_host: an inner node whose RIGHT child is node 2^24 cannot be expressed by the pair
    records (left_or_first + 1 < 2^24 is the rule), one whose right child is node 2^24 - 2 can"""
    w = cp.pool(rpt, "right_child_2^24")
    nodes = w.nodes
    inner = np.flatnonzero(nodes["triangle_count"] == 0)
    assert len(nodes) == (1 << 24) + 1 and len(nodes) % 2 == 1 and (nodes["left_or_first"][inner] % 2 == 1).all() and nodes["triangle_count"].max() == 1
    at = inner[nodes["left_or_first"][inner] == (1 << 24) - 1]
    assert len(at) == 1 and cp.tree_facts(nodes)[0] == 16
    so = hipmod.shadow_order_host(w)
    assert so["why"] == "node pool is not pair-shaped" and so["probe_rays"] == 0 and not so["fixed"]
    # the same tree with that pair two places lower
    moved = nodes.copy()
    moved[(1 << 24) - 3], moved[(1 << 24) - 2] = nodes[(1 << 24) - 1], nodes[1 << 24]
    moved[(1 << 24) - 1], moved[1 << 24] = nodes[(1 << 24) - 3], nodes[(1 << 24) - 2]
    moved["left_or_first"][at[0]] = (1 << 24) - 3
    import copy
    w2 = copy.copy(w)
    w2.nodes = moved
    assert cp.tree_facts(moved)[0] == 16
    so = hipmod.shadow_order_host(w2)
    assert so["why"] != "node pool is not pair-shaped" and so["probe_rays"] > 0
