"""Node pools at the limits of what rpt_upload_scene accepts (tests/test_chain_pools.py without a GPU, tests/test_gpu_chain_pools.py with one).  Not a test module:
the pools, their rays, a float64 brute force and a CPU model of the device's stack discipline.

chain_scene generalises extremes_scene (tests/test_gpu_walk_overhead.py): L parallel layers, layer k (1 ..) in the plane z = 40 - k, under a chain of L - 1 inner
nodes — the left child of the i-th is the leaf of layer i + 1, its right child the next inner node (the last one: the leaf of layer L).  The layers nearer z = -3 are
deeper in the chain, so a ray from (0, 0, -3) through all the boxes goes right at every node and pushes the left child: L - 1 entries, the tree's depth — the
stack of a walk that keeps the near child in hand is FULL where its capacity is the depth.  Seen from z = -3 every layer's triangle has the same angular size and its
own offset and orientation, and the two layers at either end are small, so the layer a ray hits first varies from ray to ray, from z = -3 and from z = +60: rays
that miss the near layers find their hit in a leaf that was POPPED, and an entry that comes back wrong changes an answer.  Boxes are padded by 1 / 8; child pairs stand at chosen odd indices; every other node of the pool is an unreachable leaf
of triangle 0."""
import copy

import numpy as np

import test_gpu_batch_seam as seam
from walk_rays import _aabb, restate_triangle, shadow_bounds

F = np.float32
EPS, FAR = F(0.001), F(1000000.0)
EYE_Z, BACK_Z = -3.0, 60.0
VIEW = dict(cam_position=(0.0, 0.0, EYE_Z, 0.0))
PAD = 0.125
SHADOW_RUNGS = ("t", "t-", "t+", "inf", "nan")
_cache = {}


def _layer_triangles(k, count, rng, small):
    """the triangles of layer k: ONE triangle of fixed angular size as seen from (0, 0, -3) — pointing up or down, offset by up to 0.015 rad; a `small` one 0.4 times
    that size about the axis, up in the odd layers and down in the even ones — cut into `count` slices from its apex"""
    z = 40.0 - k
    dist = z - EYE_Z
    up = 1.0 if rng.random() < 0.5 else -1.0
    off = rng.uniform(-0.015, 0.015, 2)
    scale = 1.0
    if small:
        off, scale, up = off * 0.0, 0.4, (1.0 if k % 2 else -1.0)      # (the two small layers of an end point opposite ways: neither hides the other)
    a, b, c = (np.array(p) * [scale, up * scale] + off for p in ((-0.04, -0.03), (0.04, -0.03), (0.0, 0.045)))
    out = []
    for m in range(count):
        p, q = a + (b - a) * (m / count), a + (b - a) * ((m + 1) / count)
        out.append([[p[0] * dist, p[1] * dist, z], [q[0] * dist, q[1] * dist, z], [c[0] * dist, c[1] * dist, z]])
    return out


def chain_scene(rpt, layers, lefts=None, n_nodes=None, leaf_counts=None, foreign=False, twins=None, seed=5):
    """`layers` layers under a chain of layers - 1 inner nodes: a tree of depth layers - 1.
    lefts[j]      the (odd) index of inner node j's left child; its right child stands behind it.  Default: 2j + 1, the compact pool.
    n_nodes       the pool's size; default: just large enough.  Nodes that nothing links to are leaves of triangle 0.
    leaf_counts   {layer index (0 ..): triangles in its leaf}; default one each.
    twins         {j: index}: the left child of inner node j is not the leaf of layer j but an inner node over TWO leaves (the layer has two triangles), which stand at
                  (index, index + 1).  A ray from z = -3 pushes lefts[j] at level j, and when it pops that entry and both leaves are met it writes level j again, with
                  index or index + 1: one level written twice.  (j <= layers - 3: the tree gets no deeper.)
    foreign       every pair at (even, odd) indices, as scenes.foreign_pool lays a pool out: not pair-shaped, the generic walks.
    The light is the layer nearest z = -3, turned towards the others (so that shadow probe rays can be formed)."""
    key = (layers, tuple(lefts) if lefts is not None else None, n_nodes, tuple(sorted((leaf_counts or {}).items())), foreign, tuple(sorted((twins or {}).items())), seed)
    if key in _cache:
        return _cache[key]
    L = layers
    twins = dict(twins or {})
    assert L >= 2 and all(0 <= j <= L - 3 for j in twins)
    counts = [int((leaf_counts or {}).get(i, 1)) for i in range(L)]
    for j in twins:
        assert counts[j] == 1
        counts[j] = 2
    rng = np.random.default_rng(seed)
    v, n, t = [], [], []
    for i in range(L):
        emits = i == L - 1
        for tri in _layer_triangles(i + 1, counts[i], rng, i < 2 or i >= L - 2):
            i0 = len(v)
            v += tri
            n += [[0.0, 0.0, 1.0 if emits else -1.0]] * 3
            t += [[i0, i0 + 1, i0 + 2, 3 if emits else (i % 3)]]
    w = rpt.World.from_buffers(np.array(v, F), np.array(n, F), None, np.array(t, np.uint32), seam._materials(rpt, [9.0, 8.0, 7.0, 1.0]))
    nt = len(t)
    # the builder put the triangles in ITS leaf order: back into layer order (stable), the light table's indices with them
    pos = w.per_vertex["vertex"][:, :3]
    layer = np.rint(40.0 - pos[w.indices["v0"], 2]).astype(np.int64)
    order = np.argsort(layer, kind="stable")
    inv = np.empty(nt, np.int64)
    inv[order] = np.arange(nt)
    w = copy.copy(w)
    w.indices = np.ascontiguousarray(w.indices[order])
    lp = w.light_pick.copy()
    lp["triangle_index_a"] = inv[lp["triangle_index_a"]]
    lp["triangle_index_b"] = inv[lp["triangle_index_b"]]
    w.light_pick = lp
    assert [int((np.sort(layer) == k).sum()) for k in range(1, L + 1)] == counts
    corners = np.stack([pos[w.indices[c]] for c in ("v0", "v1", "v2")], 1)                     # (nt, 3, 3)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)

    def box(f, c):
        p = corners[f:f + c].reshape(-1, 3)
        return p.min(0) - F(PAD), p.max(0) + F(PAD)

    lo, hi = zip(*[box(f, c) for f, c in zip(first, counts)])
    shift = 1 if foreign else 0
    lefts = [2 * j + 1 for j in range(L - 1)] if lefts is None else [int(x) for x in lefts]
    assert len(lefts) == L - 1 and all(x & 1 for x in lefts) and all(x & 1 for x in twins.values())
    pairs = [x + shift for x in lefts] + [x + shift for x in twins.values()]
    used = [0] + [x for p in pairs for x in (p, p + 1)]
    assert len(set(used)) == len(used), "two nodes in one place"
    nn = max(used) + 1 if n_nodes is None else int(n_nodes)
    assert nn > max(used)
    nodes = np.empty(nn, w.nodes.dtype)
    blo, bhi = box(0, 1)
    nodes["aabb_min"], nodes["aabb_max"] = blo, bhi                     # every place nothing links to: a leaf of triangle 0
    nodes["triangle_count"], nodes["left_or_first"] = 1, 0

    def leaf(at, i):
        nodes[at] = (lo[i], counts[i], hi[i], first[i])

    def layer_node(at, i):
        """layer i as one leaf, or as an inner node over its two triangles"""
        if i in twins:
            p = twins[i] + shift
            nodes[at] = (lo[i], 0, hi[i], p)
            for s in (0, 1):
                blo, bhi = box(first[i] + s, 1)
                nodes[p + s] = (blo, 1, bhi, first[i] + s)
        else:
            leaf(at, i)

    at = 0
    for j in range(L - 1):                                              # inner node j: node 0, then the right child of the one before
        p = lefts[j] + shift
        nodes[at] = (np.min(lo[j:], 0), 0, np.max(hi[j:], 0), p)
        layer_node(p, j)
        at = p + 1
    leaf(at, L - 1)
    w.nodes = nodes
    w.bvh_max_depth = L - 1
    _cache[key] = w
    return w


# ---- what a pool is, by following its links ----------------------------------------------------------------------------------------------------------------------

def tree_facts(nodes):
    """(depth of the tree under node 0, {reachable index: depth}) by following the links"""
    depth = {0: 0}
    todo = [0]
    while todo:
        i = todo.pop()
        if nodes["triangle_count"][i] == 0:
            l = int(nodes["left_or_first"][i])
            for c in (l, l + 1):
                assert c not in depth and c < len(nodes)
                depth[c] = depth[i] + 1
                todo.append(c)
    return max(depth.values()), depth


def residue_unsafe(nodes, widths=(16, 21, 24)):
    """the reachable indices i >= 2^W whose residue i mod 2^W is NOT a leaf (a library that truncates such an entry could walk in a circle), per width"""
    reach = tree_facts(nodes)[1]
    bad = []
    for W in widths:
        for i in reach:
            if i >= (1 << W) and nodes["triangle_count"][i & ((1 << W) - 1)] == 0:
                bad.append((W, i))
    return bad


def levels_written_twice(nodes):
    """[(level, first entry, second entry)] for a ray from z = -3 that meets every box: the chain pushes the left child of the inner node at depth j into level j;
    where that child is an inner node over two leaves, popping it writes level j a second time with one of its children"""
    out = []
    at, level = 0, 0
    while nodes["triangle_count"][at] == 0:
        l = int(nodes["left_or_first"][at])
        if nodes["triangle_count"][l] == 0:
            ll = int(nodes["left_or_first"][l])
            out.append((level, l, ll))
        at, level = l + 1, level + 1
    return out


# ---- the pools of the two test modules --------------------------------------------------------------------------------------------------------------------------------

def _spread(n_pairs, high_top, low_from):
    """lefts for a chain of n_pairs pairs, alternately at the top of the pool (downwards from the odd index high_top) and low (upwards from the odd index
    low_from), and the twins: one under a HIGH link standing low, one under a LOW link standing high"""
    lefts, hi_at, lo_at = [], high_top, low_from

    def next_high():
        nonlocal hi_at
        if hi_at >= 65536 and (hi_at + 1) % 65536 == 0:                 # (a pair that holds a multiple of 65 536 is left out: that index would have the root for its residue)
            hi_at -= 2
        hi_at -= 2
        return hi_at + 2

    for j in range(n_pairs):
        if j % 2 == 0:
            lefts.append(next_high())
        else:
            lefts.append(lo_at)
            lo_at += 2
    # the two levels nearest z = -3 that may hold a twin: a ray pops them after two or three leaves, so many rays come back to them with nothing hit yet
    ja, jb = sorted((n_pairs - 2, n_pairs - 3), key=lambda j: j % 2)
    twins = {ja: lo_at, jb: next_high()}                                # level ja: high entry, then low; level jb: low entry, then high
    return lefts, twins


def pool(rpt, name):
    """the named pools (tests/test_chain_pools.py says what each is for)"""
    if name.startswith("compact"):                                      # compact15 .. compact32, compact24fat, compact31fat
        d = int(name[7:9])
        return chain_scene(rpt, d + 1, leaf_counts={3: 63} if name.endswith("fat") else None)
    if name == "foreign31":
        return chain_scene(rpt, 32, foreign=True)
    if name == "sparse15_65535":                                        # width 16 at its largest entries: 65 533 and 65 534 are pushed
        lefts, twins = _spread(15, 65533, 101)
        return chain_scene(rpt, 16, lefts=lefts, n_nodes=65535, twins=twins)
    if name == "sparse15_65565":                                        # finding 1: 15 levels, links to 65 537 .. 65 564 (65 536 itself would have the root for its residue)
        lefts = [29] + [65537 + 2 * j for j in range(14)]
        return chain_scene(rpt, 16, lefts=lefts, n_nodes=65565)
    if name in ("sparse16_2m-", "sparse31_2m-"):                        # width 21, all five mask bits: entries up to 2^21 - 2
        d = int(name[6:8])
        lefts, twins = _spread(d, (1 << 21) - 3, 101)
        return chain_scene(rpt, d + 1, lefts=lefts, n_nodes=(1 << 21) - 1, twins=twins)
    if name in ("sparse16_2m+", "sparse31_2m+"):                        # width 24: entries from 2^21 + 1 on (2^21 itself would have the root for its residue)
        d = int(name[6:8])
        lefts, twins = _spread(d, (1 << 21) + 31, 101)
        return chain_scene(rpt, d + 1, lefts=lefts, n_nodes=(1 << 21) + 33, twins=twins)
    if name == "right_child_2^24":                                      # section 6: an inner node whose right child is node 2^24
        lefts = [2 * j + 1 for j in range(16)]
        lefts[1] = (1 << 24) - 1                                        # (near the root: the rays from z = +60 that miss layer 1 push node 2^24 there)
        return chain_scene(rpt, 17, lefts=lefts, n_nodes=(1 << 24) + 1)
    raise KeyError(name)


SMALL_POOLS = ("compact15", "compact16", "compact23", "compact24", "compact31", "compact24fat", "compact31fat", "foreign31", "sparse15_65535", "sparse15_65565")
LARGE_POOLS = ("sparse16_2m-", "sparse31_2m-", "sparse16_2m+", "sparse31_2m+")
POOLS = SMALL_POOLS + LARGE_POOLS


# ---- rays ---------------------------------------------------------------------------------------------------------------------------------------------------------

def bundle(from_z, n=4096, seed=41):
    """n rays from (0, 0, from_z) towards the layers, N(0, 0.02) about the axis"""
    rng = np.random.default_rng(seed + (0 if from_z < 0 else 1))
    o = np.tile(np.array([[0.0, 0.0, from_z]], F), (n, 1))
    d = np.tile(np.array([[0.0, 0.0, 1.0 if from_z < 20 else -1.0]], F), (n, 1))
    d[:, :2] += rng.normal(size=(n, 2)).astype(F) * F(0.02)
    return o, d


def nearest_rays():
    """both bundles: 8 192 rays"""
    (o1, d1), (o2, d2) = bundle(EYE_Z), bundle(BACK_Z)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


def shadow_rays(t_of, n_each=800):
    """the first n_each rays of each bundle under the rungs t, t-, t+, inf, nan of walk_rays.shadow_bounds: (origins, directions, max_t), 8 000 rays.
    t_of(o, d): the nearest accepted t of each ray (the oracle's)"""
    (o1, d1), (o2, d2) = bundle(EYE_Z), bundle(BACK_Z)
    o, d = np.concatenate([o1[:n_each], o2[:n_each]]), np.concatenate([d1[:n_each], d2[:n_each]])
    ladder = dict(shadow_bounds(t_of(o, d)))
    return np.tile(o, (len(SHADOW_RUNGS), 1)), np.tile(d, (len(SHADOW_RUNGS), 1)), np.concatenate([ladder[g] for g in SHADOW_RUNGS])


# ---- Moller-Trumbore over ALL triangles in float64 ------------------------------------------------------------------------------------------------------------------

def brute_force(w, o, d):
    """(hit, t, triangle, smallest barycentric distance to an edge of any triangle whose plane the ray meets in front of it) in float64, with the reference's four
    rejections (|det| < 1e-6; u < 0 or u > 1; v < 0 or u + v > 1; t < 0) and t > 0.001"""
    pos = w.per_vertex["vertex"][:, :3].astype(np.float64)
    a, b, c = (pos[w.indices[k]] for k in ("v0", "v1", "v2"))
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = len(o)
    best, tri, hit, edge = np.full(n, 1.0e6), np.zeros(n, np.int64), np.zeros(n, bool), np.full(n, np.inf)
    for k in range(len(a)):
        e1, e2 = b[k] - a[k], c[k] - a[k]
        pv = np.cross(d, e2)
        det = pv @ e1
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            tv = o - a[k]
            u = (tv * pv).sum(1) * inv
            qv = np.cross(tv, e1)
            v = (d * qv).sum(1) * inv
            t = (qv @ e2) * inv
            ok = ~(np.abs(det) < 1e-6) & ~((u < 0) | (u > 1)) & ~((v < 0) | (u + v > 1)) & ~(t < 0) & (t > 0.001)
            near_edge = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(1.0 - u - v))
            edge = np.where(t > 0.001, np.minimum(edge, near_edge), edge)
        acc = ok & (t < best)
        best, tri, hit = np.where(acc, t, best), np.where(acc, k, tri), hit | acc
    return hit, best, tri, edge


# ---- the device's stack discipline, on the CPU -----------------------------------------------------------------------------------------------------------------------

def walk_model(world, o, d, entry_bits, capacity, clears_stale_bits=True, step_limit=4096):
    """The nearest-hit walk as the device's global-memory kernels make it (csrc/k_walk.h walk_run), every ray in step, in float32 numpy: the reference's visiting order
    (intersection.rs:177-234: both children tested against the best t so far, the nearer entered, ties to the left) with the near child kept in hand and the FAR
    child's node index stored at its level — masked to entry_bits, in `capacity` levels (a push beyond them is dropped, as the kernels' `sp < STACK` drops it);
    entry_bits 21 keeps a 16-bit word and five mask bits per level, which a push clears before it sets them unless clears_stale_bits is False.  A popped index
    outside the pool ends its ray.  Returns (hit, t, triangle, back face, finished): `finished` False for a ray still walking after step_limit steps or sent outside
    the pool."""
    nodes = world.nodes
    nn = len(nodes)
    count, link = nodes["triangle_count"].astype(np.int64), nodes["left_or_first"].astype(np.int64)
    lo, hi = nodes["aabb_min"].astype(F), nodes["aabb_max"].astype(F)
    pos = world.per_vertex["vertex"][:, :3].astype(F)
    ta, tb, tc = (pos[world.indices[k]] for k in ("v0", "v1", "v2"))
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    n = len(o)
    cur, sp = np.zeros(n, np.int64), np.zeros(n, np.int64)
    word = np.zeros((n, capacity), np.int64)                            # the 16-bit column (the whole entry for the other widths)
    bits = np.zeros((n, capacity), np.int64)                            # width 21: bit 16 + k of a level's entry, as the five mask registers hold it
    best, tri, back, hit = np.full(n, FAR, F), np.zeros(n, np.uint32), np.zeros(n, bool), np.zeros(n, bool)
    alive, lost = np.ones(n, bool), np.zeros(n, bool)
    mask = (1 << entry_bits) - 1

    def pop(rows):
        """rows: indices of rays that have nothing in hand"""
        empty = sp[rows] == 0
        alive[rows[empty]] = False
        r = rows[~empty]
        sp[r] -= 1
        e = word[r, sp[r]] | bits[r, sp[r]]
        outside = e >= nn
        lost[r[outside]] = True
        alive[r[outside]] = False
        cur[r[~outside]] = e[~outside]

    for _ in range(step_limit):
        rows = np.flatnonzero(alive)
        if len(rows) == 0:
            break
        inner = rows[count[cur[rows]] == 0]
        leaves = rows[count[cur[rows]] != 0]
        if len(inner):
            l = link[cur[inner]]
            r = l + 1
            tl = _aabb(lo[l], hi[l], o[inner], d[inner], best[inner])
            tr = _aabb(lo[r], hi[r], o[inner], d[inner], best[inner])
            hl, hr = ~np.isinf(tl), ~np.isinf(tr)
            swap = hr & (~hl | (tl > tr))
            both = hl & hr
            push = both & (sp[inner] < capacity)
            pr = inner[push]
            far = np.where(swap[push], l[push], r[push]) & mask
            if entry_bits == 21:
                word[pr, sp[pr]] = far & 0xFFFF
                bits[pr, sp[pr]] = (far & ~0xFFFF) | (0 if clears_stale_bits else bits[pr, sp[pr]])
            else:
                word[pr, sp[pr]] = far
            sp[pr] += 1
            any_ = hl | hr
            cur[inner[any_]] = np.where(swap[any_], r[any_], l[any_])
            pop(inner[~any_])
        if len(leaves):
            c, f = count[cur[leaves]], link[cur[leaves]]
            for i in range(int(c.max())):
                m = c > i
                rr, k = leaves[m], f[m] + i
                passes, det, _, _, t = restate_triangle(o[rr], d[rr], ta[k], tb[k], tc[k])
                with np.errstate(all="ignore"):
                    acc = passes & (t > EPS) & (t < best[rr])
                ar = rr[acc]
                best[ar], tri[ar], back[ar], hit[ar] = t[acc], k[acc], np.signbit(det[acc]), True
            pop(leaves)
    return hit, best, tri, back, ~(alive | lost)


def library_choice(w):
    """(capacity, entry bits) that the library is meant to choose for a pair-shaped pool with no RPT_STACK_BITS (rpt_scene.hip where stack_cap is set, rpt_traverse.hip
    gstream_stack_width); a pool that is not pair-shaped: the generic walks, 32 entries of 32 bits"""
    depth, reach = tree_facts(w.nodes)
    nn = len(w.nodes)
    inner = w.nodes["triangle_count"] == 0
    pair_shaped = nn % 2 == 1 and bool(np.all(w.nodes["left_or_first"][inner] % 2 == 1)) and int(w.nodes["left_or_first"][inner].max()) + 1 < (1 << 24)
    if not pair_shaped:
        return 32, 32
    cap = 16 if depth <= 15 and nn < 65536 else (24 if depth <= 23 else 32)
    bits = 16 if nn < 65536 else (21 if nn < (1 << 21) else (24 if nn < (1 << 24) else 32))
    return cap, (16 if cap == 16 else min(bits, 24) if cap == 24 else bits)
