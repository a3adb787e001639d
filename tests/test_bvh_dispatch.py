"""Every split path of the device BVH build is witnessed by one case (tests/bvh_cases.py): asserted here on the ORACLE's trees alone, so that the GPU
test that builds the same case (tests/test_gpu_bvh_build.py::test_gpu_build_down_every_split_path) is known to have run all five split kernels, their
size boundaries, a multi-trip counting pass and team chunks on both sides of a workgroup's width."""
import numpy as np
import pytest

import bvh_cases
from bvh_cases import BVB_RUN, DISPATCH_BINS, PATHS, dispatch_case, split_paths


@pytest.fixture(scope="module")
def trees(oracle):
    return dispatch_case(oracle)[2]


def test_split_paths_on_a_tree_worked_by_hand():
    """Seven triangles, root split 4 | 3, the left child 2 | 2: one level<1024> level after another (fewer than 64 nodes), a team at the root once the
    threshold lets it, and nothing for the leaves."""
    z = [0, 0, 0]
    pool = np.array([z + [0] + z + [1], z + [0] + z + [3], z + [3] + z + [4], z + [2] + z + [0], z + [2] + z + [2]], np.uint32)
    depth, count, inner = bvh_cases.tree_levels(pool)
    assert depth.tolist() == [0, 1, 1, 2, 2] and count.tolist() == [7, 4, 3, 2, 2] and inner.tolist() == [True, True, False, False, False]
    got = split_paths(pool)
    assert got["level<1024>"] == [(7, 4, 1), (4, 2, 2)] and all(got[p] == [] for p in PATHS if p != "level<1024>")
    got = split_paths(pool, team_min=5)
    assert got["team"] == [(7, 4, 1)] and got["team_sizes"] == [(7, 2)] and got["level<1024>"] == [(4, 2, 2)]


@pytest.mark.parametrize("bins", DISPATCH_BINS)
def test_every_split_kernel_splits_a_node(trees, bins):
    got = split_paths(trees[bins][0])
    for path in PATHS:                                          # (the team too: the root)
        assert any(0 < left < n for n, left, _ in got[path]), path
    assert got["team or level<1024>"] == []


@pytest.mark.parametrize("bins", DISPATCH_BINS)
def test_one_wave_kernels_meet_their_size_limits(trees, bins):
    """8 | 9: k_bvb_tiny's last size and the first it leaves to the launch behind it; 64 | 65: k_bvb_small's last size and the first only k_bvb_level<64>
    takes — all on levels of 64 or more nodes, where the host picks kernels by size at all."""
    got = split_paths(trees[bins][0])
    at = {path: {n for n, _, level in got[path] if level >= 64} for path in PATHS}
    assert 8 in at["tiny"]
    assert 9 in at["small"] and 9 in at["level<64>"]
    assert 64 in at["small"] | at["level<64>"]
    assert 65 in at["level<64>"]


@pytest.mark.parametrize("bins", DISPATCH_BINS)
def test_counting_pass_takes_more_than_one_trip(trees, bins):
    got = split_paths(trees[bins][0])
    assert max(n for n, _, _ in got["level<256>"]) > BVB_RUN * 256 == 1024


def test_small_teams_on_both_sides_of_a_workgroups_width(trees):
    """RPT_BVH_TEAM_MIN=2: two-workgroup teams whose chunk, ceil(count / 2), is shorter than the 256 threads that walk it, exactly as long, and longer."""
    chunks = {}
    for bins in DISPATCH_BINS:
        got = split_paths(trees[bins][0], team_min=2)
        split = {n for n, left, _ in got["team"] if 0 < left < n}
        chunks[bins] = {(n + 1) // 2 for n, size in got["team_sizes"] if size == 2 and n in split}
        assert min(chunks[bins]) < 256 < max(chunks[bins])
    assert any(256 in c for c in chunks.values())
