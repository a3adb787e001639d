"""Chosen rays for the production walk kernels (rpt_debug_walk_production; tests/test_walk_production_rays.py without a GPU, tests/test_gpu_walk_production.py with
one).  Not a test module: the ray sets, and a float32 numpy restatement of the reference's walk over the two-leaf scene of tests/test_gpu_walk_scalar.py —
intersect_aabb, muller_trumbore and the acceptance of intersection.rs:177-234 operation by operation — that can also be run with ONE comparison changed (NEAR_MISSES):
the CPU tests count the rays of the sets whose answer such a nearly right walk changes, in the place of planting wrong kernels on a GPU."""
import numpy as np

from test_anyhit_order import _shadow_like_rays  # noqa: F401
from test_gpu_walk_overhead import extremes_scene  # noqa: F401
from test_gpu_walk_scalar import TRIS, _dirs, bound_rays, one_triangle_scene, restate, special_rays, two_leaf_scene  # noqa: F401

F = np.float32
EPS, FAR = F(0.001), F(1000000.0)
_cache = {}

# rays in a shadow queue: one; fewer than a streamed wave refills for (RPT_STREAM_REFILL = 16, k_walk_stream.h); around one wave; around a chunk of a shard (256 entries,
# k_common.h); more than one workgroup of the loader and more than a shard's first chunk in every shard
QUEUE_SHAPES = (1, 15, 63, 64, 65, 255, 257, 4097)


# ---- max_t ---------------------------------------------------------------------------------------------------------------------------------------------------

RUNGS = ("t", "t-", "t+", "1e6-", "1e6", "2e6", "inf", "nan", "0", "-0", "-1", "1e-45", "0.001-", "0.001", "0.001+")
UNBOUNDED = ("1e6", "2e6", "inf")                 # from 1e6 on a bound bounds nothing: the walk accepts t < 1e6 only
NOTHING = ("nan", "0", "-0", "-1", "1e-45", "0.001-", "0.001")   # t <= NaN never holds, and t > 0.001 leaves nothing at or below it


def shadow_bounds(t):
    """the ladder of max_t for rays whose nearest accepted t is `t`: [(rung, max_t per ray)] in the order of RUNGS"""
    t = np.ascontiguousarray(t, F)
    full = lambda x: np.full(len(t), x, F)
    with np.errstate(all="ignore"):
        out = [t.copy(), np.nextafter(t, F(0)), np.nextafter(t, F(np.inf)), full(np.nextafter(FAR, F(0))), full(FAR), full(2.0e6), full(np.inf), full(np.nan),
               full(0.0), full(-0.0), full(-1.0), full(1e-45), full(np.nextafter(EPS, F(0))), full(EPS), full(np.nextafter(EPS, F(1)))]
    return list(zip(RUNGS, out))


# ---- the reference's walk over the two-leaf scene, in float32 numpy ---------------------------------------------------------------------------------------------

NEAR_MISSES = ("t < max_t", "t >= 0.001", "|det| <= 1e-6", "u + v >= 1 rejected", "back faces rejected", "NaN max_t accepts", "max_t >= 1e6 bounds")
_LEAF_BOXES = [(TRIS[:2].reshape(-1, 3).min(0), TRIS[:2].reshape(-1, 3).max(0)), (TRIS[2:].reshape(-1, 3).min(0), TRIS[2:].reshape(-1, 3).max(0))]


def restate_triangle(o, d, a, b, c):
    """tests/test_gpu_walk_scalar.py restate for ANY triangle (a, b, c: one triangle or one per ray): (passes the Moller-Trumbore test, det, u, v, t)"""
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    a, b, c = (np.broadcast_to(np.asarray(x, F), o.shape) for x in (a, b, c))
    cross = lambda p, q: np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], 1).astype(F)
    dot = lambda p, q: ((p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1]).astype(F) + p[:, 2] * q[:, 2]).astype(F)
    with np.errstate(all="ignore"):
        e1, e2 = (b - a).astype(F), (c - a).astype(F)
        pv = cross(d, e2)
        det = dot(e1, pv)
        inv = (F(1.0) / det).astype(F)
        tv = (o - a).astype(F)
        u = (dot(tv, pv) * inv).astype(F)
        qv = cross(tv, e1)
        v = (dot(d, qv) * inv).astype(F)
        t = (dot(e2, qv) * inv).astype(F)
        passes = ~(np.abs(det) < F(1e-6)) & ~((u < 0) | (u > 1)) & ~((v < 0) | ((u + v).astype(F) > 1)) & ~(t < 0)
    return passes, det, u, v, t


def _passes(det, u, v, t, miss):
    """muller_trumbore's four early-outs, each written as the reference writes it (a NaN falls through every one)"""
    with np.errstate(all="ignore"):
        small = (np.abs(det) <= F(1e-6)) if miss == "|det| <= 1e-6" else (np.abs(det) < F(1e-6))
        sum_out = ((u + v).astype(F) >= 1) if miss == "u + v >= 1 rejected" else ((u + v).astype(F) > 1)
        ok = ~small & ~((u < 0) | (u > 1)) & ~((v < 0) | sum_out) & ~(t < 0)
        if miss == "back faces rejected":
            ok &= ~np.signbit(det)
    return ok


def _aabb(lo, hi, o, d, prev):
    """intersect_aabb (intersection.rs:104-122): tmin, or +inf where the box is not entered"""
    with np.errstate(all="ignore"):
        t1, t2 = ((lo - o).astype(F) / d).astype(F), ((hi - o).astype(F) / d).astype(F)
        mn, mx = np.fmin(t1, t2), np.fmax(t1, t2)
        tmin = np.fmax(np.fmax(mn[:, 0], mn[:, 1]), mn[:, 2])
        tmax = np.fmin(np.fmin(mx[:, 0], mx[:, 1]), mx[:, 2])
        ok = (tmax >= tmin) & (tmax > 0) & (tmin < prev)
    return np.where(ok, tmin, F(np.inf)).astype(F)


def walk_two_leaf(o, d, max_t=None, miss=None):
    """intersect_front_to_back over the two-leaf scene.  max_t None: the nearest hit, (hit, t, triangle, backface) as oracle.trace_rays(kind 0) reports them;
    else `.hit` of the any-hit walk.  miss: one of NEAR_MISSES, the comparison a nearly right walk would get wrong."""
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    n = len(o)
    ok, ts, back = [], [], []
    for k in range(3):
        _, det, u, v, t = restate(o, d, np.full(n, k))
        ok.append(_passes(det, u, v, t, miss))
        ts.append(t)
        back.append(np.signbit(det))
    ok, ts, back = np.stack(ok, 1), np.stack(ts, 1), np.stack(back, 1)
    with np.errstate(all="ignore"):
        above = (ts >= EPS) if miss == "t >= 0.001" else (ts > EPS)
        if max_t is not None:
            max_t = np.ascontiguousarray(max_t, F)
            # what every t is compared against before anything is accepted: result.t = 1e6 (a bound from 1e6 on in its place: the near miss of a walk that
            # takes max_t for that constant, as the segment-bounded walks do with a bound below it)
            limit = np.where(max_t >= FAR, np.nextafter(max_t, F(np.inf)), FAR).astype(F) if miss == "max_t >= 1e6 bounds" else np.full(n, FAR, F)
            enter = np.stack([~np.isinf(_aabb(lo, hi, o, d, limit)) for lo, hi in _LEAF_BOXES], 1)[:, [0, 0, 1]]
            within = (ts < max_t[:, None]) if miss == "t < max_t" else (ts <= max_t[:, None])
            if miss == "NaN max_t accepts":
                within |= np.isnan(max_t)[:, None]
            return (enter & ok & above & (ts < limit[:, None]) & within).any(axis=1)
        da, db = (_aabb(lo, hi, o, d, FAR) for lo, hi in _LEAF_BOXES)
        b_first = da > db                                                              # (the reference swaps when min_dist > max_dist)
        seq = np.where(b_first[:, None], np.array([2, 0, 1]), np.array([0, 1, 2]))      # the triangles in the order they are tested
        entered = np.stack([~np.isinf(da), ~np.isinf(da), ~np.isinf(db)], 1)            # a pushed leaf is popped without another box test
        best, tri, bf, hit = np.full(n, FAR, F), np.zeros(n, np.uint32), np.zeros(n, bool), np.zeros(n, bool)
        rows = np.arange(n)
        for j in range(3):
            k = seq[:, j]
            acc = entered[rows, k] & ok[rows, k] & above[rows, k] & (ts[rows, k] < best)
            best = np.where(acc, ts[rows, k], best).astype(F)
            tri = np.where(acc, k, tri).astype(np.uint32)
            bf = np.where(acc, back[rows, k], bf)
            hit |= acc
    return hit, best, tri, bf


# ---- rays for the max_t ladder ----------------------------------------------------------------------------------------------------------------------------------

def ladder_rays():
    """bound_rays() and three classes it lacks, (origins, directions, aimed triangle, class): rays whose t is 0.001 to the bit, and the float above it (T0: the
    plane z = 0 and d.z = 1 leave nothing to round), and rays that pass T1's test at t = 2^20 >= 1e6 after entering its leaf's box at 2^19 (accepted by no walk
    that keeps the reference's 1e6)"""
    if "ladder" in _cache:
        return _cache["ladder"]
    o, d, tri, cls = bound_rays()
    rng = np.random.default_rng(23)
    g = np.arange(1, 16) / 16.0
    uv = np.array([(x, y) for x in g[::2] for y in g[::2] if x + y < 1], np.float64)

    def through(k, s, scale):
        a, e1, e2 = (TRIS[k, 0].astype(np.float64), (TRIS[k, 1] - TRIS[k, 0]).astype(np.float64), (TRIS[k, 2] - TRIS[k, 0]).astype(np.float64))
        p = a + uv[:, :1] * e1 + uv[:, 1:] * e2
        dd = _dirs(rng, len(uv)).astype(np.float64)
        return (p - s * dd).astype(F), (dd * scale).astype(F)

    above = float(np.nextafter(EPS, F(1)))
    parts = [(*through(0, float(EPS), 1.0), 0, "t == 0.001"), (*through(0, float(EPS), 1.0), 0, "t == 0.001"),
             (*through(0, above, 1.0), 0, "t == 0.001+"), (*through(0, above, 1.0), 0, "t == 0.001+"),
             (*through(1, 2.0, 2.0 ** -19), 1, "t >= 1e6"), (*through(1, 2.0, 2.0 ** -19), 1, "t >= 1e6")]
    o = np.concatenate([o] + [p[0] for p in parts])
    d = np.concatenate([d] + [p[1] for p in parts])
    tri = np.concatenate([tri] + [np.full(len(p[0]), p[2]) for p in parts])
    cls = np.concatenate([cls] + [np.array([p[3]] * len(p[0])) for p in parts])
    _cache["ladder"] = (o, d, tri, cls)
    return _cache["ladder"]


# ---- FIRST: every ray from one origin ---------------------------------------------------------------------------------------------------------------------------

# inside the root's box; outside it; 1e4 away, where `plane - origin` rounds (the FIRST walk stages exactly that difference); y on a plane of both leaves' boxes
# (slab distance 0); a zero coordinate
FAN_ORIGINS = {"inside": (2.25, 0.5, 0.5), "outside": (1.1, 0.3, -3.2), "far": (-8190.3, 0.4, -8191.7), "on a box plane": (1.7, 1.0, -2.3), "zero coordinate": (0.0, 0.45, -2.6)}
FAN_CLASSES = ("vertex", "edge", "just inside", "just outside", "random")


def two_leaf_points():
    """(points, the triangle each lies in the plane of, class): the bounds of the three triangle tests as points in space"""
    g = np.arange(1, 16) / 16.0
    step = 1.0 / 64
    p, tri, cls = [], [], []
    for k in range(3):
        a, e1, e2 = (TRIS[k, 0].astype(np.float64), (TRIS[k, 1] - TRIS[k, 0]).astype(np.float64), (TRIS[k, 2] - TRIS[k, 0]).astype(np.float64))
        sets = {"vertex": [(0, 0), (1, 0), (0, 1)] * 8,
                "edge": [(0, y) for y in g] + [(x, 0) for x in g] + [(x, 1 - x) for x in g],
                "just inside": [(step, y) for y in g[:14]] + [(x, step) for x in g[:14]] + [(x, 1 - x - step) for x in g[1:14]],
                "just outside": [(-step, y) for y in g] + [(x, -step) for x in g] + [(x, 1 - x + step) for x in g]}
        for name, uv in sets.items():
            uv = np.array(uv, np.float64)
            p.append(a + uv[:, :1] * e1 + uv[:, 1:] * e2)
            tri.append(np.full(len(uv), k))
            cls += [name] * len(uv)
    return np.concatenate(p), np.concatenate(tri), np.array(cls)


def fan(origin, points, n_random=512, seed=29):
    """(origins, directions): one origin (float32, repeated), directions towards `points` — scaled so that their largest component is 1, inside the exact-division
    guard, each point a second and third time with one component of the direction a few floats up or down — and n_random directions towards the lines through
    two of the points.  What each ray meets is for the caller to COMPUTE: from a common origin no barycentric lands on 0 or 1 by construction."""
    rng = np.random.default_rng(seed)
    origin = np.asarray(origin, F)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    d = points - origin.astype(np.float64)
    d = (d / np.abs(d).max(axis=1, keepdims=True)).astype(F)
    up, down = d.copy(), d.copy()
    rows = np.arange(len(d))
    axis = rows % 3
    for step in range(3):                                                               # one to three floats, by the point's place in the list
        more = (rows // 3) % 3 >= step
        up[rows[more], axis[more]] = np.nextafter(up[rows[more], axis[more]], F(np.inf))
        down[rows[more], axis[more]] = np.nextafter(down[rows[more], axis[more]], F(-np.inf))
    a, b = points[rng.integers(0, len(points), n_random)], points[rng.integers(0, len(points), n_random)]
    rnd = a + rng.uniform(-0.5, 1.5, (n_random, 1)) * (b - a) - origin.astype(np.float64)      # on and beyond the lines between two of the points
    rnd = (rnd / np.abs(rnd).max(axis=1, keepdims=True)).astype(F)
    rnd[rnd == 0] = F(2.0 ** -20)
    d = np.concatenate([d, up, down, rnd])
    return np.tile(origin, (len(d), 1)), np.ascontiguousarray(d)


def two_leaf_fan(name):
    """fan(FAN_ORIGINS[name], two_leaf_points()) with what it was built for: (origins, directions, aimed triangle or -1, class)"""
    if ("fan", name) not in _cache:
        p, tri, cls = two_leaf_points()
        o, d = fan(FAN_ORIGINS[name], p)
        n_rnd = len(o) - 3 * len(p)
        _cache[("fan", name)] = (o, d, np.concatenate([tri, tri, tri, np.full(n_rnd, -1)]), np.concatenate([cls, cls, cls, np.array(["random"] * n_rnd)]))
    return _cache[("fan", name)]
