"""Which kernel of the device BVH build (csrc/k_bvh_build.h) splits which node, restated on the CPU from a finished tree, and the one soup whose tree
sends work down every one of those paths (tests/test_bvh_dispatch.py asserts that on the oracle's tree; tests/test_gpu_bvh_build.py builds it on the device).

A level of the device build is exactly the nodes of one depth of the finished tree, so the host's choice of kernels per level (csrc/rpt_bvh.hip,
rpt_bvh_build_gpu: bvb_launch_level and the team block in front of it) follows from the oracle's node pool alone."""
import numpy as np

# csrc/k_bvh_build.h
BVB_TINY = 8                    # k_bvb_tiny: nodes of up to 8 triangles
BVB_TEAM = 256                  # the largest team
BVB_TEAM_CHUNK = 8192           # triangles per workgroup a team is sized for
BVB_MAX_TEAMS = 128             # teams per launch
BVB_TEAM_MIN_COUNT = 16384      # RPT_BVH_TEAM_MIN unset
BVB_WIDE_MIN_COUNT = 16384
BVB_RUN = 4                     # bvb_count_left: positions per thread and trip

PATHS = ("team", "level<1024>", "level<256>", "level<64>", "small", "tiny")


def tree_levels(nodes):
    """(depth, triangles, is_inner) per node of an oracle node pool ((n, 8) uint32 words: min x y z, triangle_count, max x y z, left_or_first).
    The reference numbers children after their parent (bvh.rs:296-320), the right child is left + 1."""
    nodes = np.asarray(nodes).view(np.uint32).reshape(-1, 8)
    n = len(nodes)
    count = nodes[:, 3].astype(np.int64)
    left = nodes[:, 7].astype(np.int64)
    inner = count == 0
    depth = np.zeros(n, np.int64)
    for i in range(n):
        if inner[i]:
            assert i < left[i] < n - 1
            depth[left[i]] = depth[left[i] + 1] = depth[i] + 1
    for i in range(n - 1, -1, -1):
        if inner[i]:
            count[i] = count[left[i]] + count[left[i] + 1]
    return depth, count, inner


def team_size(count, room):
    """rpt_bvh_build_gpu's sizing of one team (the two `while (size ...` lines of its team block): a power of two of workgroups, one per
    BVB_TEAM_CHUNK triangles, halved until it fits the room left in the launch; 0: no room."""
    size = 2
    while size < BVB_TEAM and size * BVB_TEAM_CHUNK < count:
        size *= 2
    while size > 2 and size > room:
        size //= 2
    return size if size <= room else 0


def split_paths(nodes, team_min=BVB_TEAM_MIN_COUNT, resident=256):
    """{path: [(triangles, triangles of the left child, nodes in the level), ...]} over the nodes the device build SPLITS (the inner nodes of the
    tree), by the kernel that splits them, and under "team_sizes" the (triangles, workgroups) of every team.  Mirrors rpt_bvh_build_gpu's loop
    `while (begin < end)` in csrc/rpt_bvh.hip:
      - the team block (`if (resident >= 2u && end - begin <= 4096u && level_max >= team_min)`): nodes of at least team_min triangles, at most
        BVB_MAX_TEAMS of them and `resident` workgroups in all, are split by k_bvb_team and skipped by the launches that follow (pad[0]);
        `resident` is what the device holds of k_bvb_team at once — one workgroup per CU of an MI355X is the least it can be with teams on at all;
      - bvb_launch_level: fewer than 64 nodes in the level, or level_max >= BVB_WIDE_MIN_COUNT: k_bvb_level<1024>; level_max <= 256: k_bvb_tiny
        for the nodes of up to BVB_TINY triangles, then k_bvb_small (level_max <= 64) or k_bvb_level<64> for the others; else k_bvb_level<256>;
      - `level_max = teams_here ? nt : total[1]`: the largest node of the level, but the whole scene's size after a level on which teams ran.
    Which nodes get a team when a level has more candidates than fit in one launch depends on the order the level was numbered in, which is the order
    the atomics of the level above landed in: the candidates of such a level are listed under "team or level<1024>" (after teams, level_max is the
    whole scene's size) and under no path."""
    depth, count, inner = tree_levels(nodes)
    left = np.asarray(nodes).view(np.uint32).reshape(-1, 8)[:, 7].astype(np.int64)
    nt = int(count[0])
    out = {p: [] for p in PATHS + ("team or level<1024>",)}
    out["team_sizes"] = []
    level_max = nt
    for d in range(int(depth.max()) + 1):
        ids = np.flatnonzero(depth == d)
        n_level = len(ids)
        taken, unsure = set(), set()
        teams_here = False
        if resident >= 2 and n_level <= 4096 and level_max >= team_min:
            wanted = [int(i) for i in ids if count[i] >= team_min]
            sizes = [team_size(int(count[i]), resident) for i in wanted]
            teams_here = len(wanted) > 0
            if len(wanted) > BVB_MAX_TEAMS or sum(sizes) > resident:
                unsure = set(wanted)
            else:
                taken = set(wanted)
                out["team_sizes"] += [(int(count[i]), s) for i, s in zip(wanted, sizes)]
        for i in ids:
            c = int(count[i])
            if int(i) in unsure:
                path = "team or level<1024>"
            elif int(i) in taken:
                path = "team"
            elif n_level < 64 or level_max >= BVB_WIDE_MIN_COUNT:
                path = "level<1024>"
            elif level_max <= 256:
                path = "tiny" if c <= BVB_TINY else ("small" if level_max <= 64 else "level<64>")
            else:
                path = "level<256>"
            if inner[i]:
                out[path].append((c, int(count[left[i]]), n_level))
        level_max = nt if teams_here else max([max(int(count[left[i]]), int(count[left[i] + 1])) for i in ids if inner[i]], default=0)
    return out


DISPATCH_BINS = (3, 128)
DISPATCH_SEED = 11              # chosen on the oracle's trees alone, so that every assertion of tests/test_bvh_dispatch.py holds


def dispatch_soup(seed=DISPATCH_SEED, n=40_000):
    """(vertices (3n, 4) float32, n triangles): small triangles in clusters of very different sizes and densities over a thin uniform background, shuffled —
    the tree has big and small nodes side by side on its middle levels."""
    from importlib import import_module
    ffi = import_module("rust-path-tracer_amd._ffi")
    rng = np.random.default_rng(seed)
    k = 24
    centres = rng.uniform(-10.0, 10.0, (k, 3))
    radius = rng.choice([0.05, 0.3, 1.0, 3.0], k)
    weight = rng.random(k) ** 3
    which = rng.choice(k, n, p=weight / weight.sum())
    c = centres[which] + rng.normal(size=(n, 3)) * radius[which][:, None]
    background = rng.random(n) < 0.1
    c[background] = rng.uniform(-12.0, 12.0, (int(background.sum()), 3))
    p = (c[:, None, :] + rng.normal(size=(n, 3, 3)) * 0.01).astype(np.float32)
    v = np.concatenate([p.reshape(-1, 3), np.ones((3 * n, 1), np.float32)], 1)
    t = np.zeros(n, ffi.TRIANGLE_DTYPE)
    idx = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    t["v0"], t["v1"], t["v2"] = idx[:, 0], idx[:, 1], idx[:, 2]
    return v, t[rng.permutation(n)]


_case = {}


def dispatch_case(oracle):
    """(vertices, triangles, {bins: (oracle nodes, oracle triangles)}) of the dispatch soup, built once per process."""
    if not _case:
        v, t = dispatch_soup()
        _case["v"], _case["t"] = v, t
        _case["built"] = {bins: oracle.bvh_build(v, t, bins) for bins in DISPATCH_BINS}
    return _case["v"], _case["t"], _case["built"]
