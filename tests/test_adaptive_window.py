"""The window rule of rpt_render_adaptive_window without a GPU: the host build of csrc/k_adaptive.h (rpt_debug_adaptive_window_host: the row words, shifts and ORs
the kernel k_ad_window runs, tile by tile) against the numpy restatement of tests/adaptive_window_ref.py (shifted boolean images), on real and hostile records;
the tile clip, the order of window and cap, the independence from the partition, the pass schedule, the refusals, and the recommended radius against the kept
grid."""
import os
import re

import numpy as np
import pytest

import adaptive_ref as aref
import adaptive_window_ref as awr
import moments_ref as ref

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(37, 23), (64, 64), (65, 65), (130, 67), (100, 70)]      # one partial tile; one exact tile; tiles one pixel wide and high; 3 x 2 tiles, last 2 wide / 3 tall
RADII = [0, 1, 2, 3, 8]                                            # 8 exceeds the extent of the small tiles


def quiet(h, w, count=16):
    """records at or below every threshold: `count` equal samples (zero variance), so that whatever is selected was planted"""
    m = np.zeros((h, w, 4), F)
    m[..., 0], m[..., 1], m[..., 2], m[..., 3] = F(0.5) * count, F(0.25) * count, count, F(0.5)
    return m


def hostile_image(w, h, seed, share):
    """(h, w, 4) records: quiet ones, and a `share` of plausible noisy ones and hostile ones — NaN and +-inf in any word, n of 0, 1, 2 and 2^24, counts at and
    next to the cap, negative sums, zero variance"""
    g = np.random.default_rng(seed)
    n = w * h
    count = g.integers(2, 70, n).astype(F)
    mean = g.gamma(0.5, 2.0, n).astype(F)
    spread = (g.random(n) ** 4).astype(F) * F(3)
    m = np.zeros((n, 4), F)
    m[:, 0], m[:, 1], m[:, 2], m[:, 3] = mean * count, (mean * mean * (F(1) + spread)) * count, count, mean * F(2)
    kind = g.integers(0, 16, n)
    for k, word in ((0, 0), (1, 1), (2, 2), (3, 3)):
        at = np.flatnonzero(kind == k)
        m[at, word] = g.choice(np.array([np.nan, np.inf, -np.inf], F), len(at))
    at = np.flatnonzero(kind == 4)
    m[at, 2] = g.choice(np.array([0, 1, 2, 2 ** 24, 56, 57, 64], F), len(at))
    m[kind == 5, 0] *= F(-1)                                                # a negative sum
    m[kind == 6, 1] = F(-1)                                                 # a negative sum of squares
    m[kind == 7, 1] = m[kind == 7, 0] * m[kind == 7, 0] / m[kind == 7, 2]   # zero (or rounding-negative) variance
    m[kind == 8, :2] = 0                                                    # a black pixel
    out = quiet(h, w, 16).reshape(n, 4)
    planted = g.random(n) < share
    out[planted] = m[planted]
    return out.reshape(h, w, 4)


@pytest.mark.parametrize("w,h", SIZES)
def test_host_window_is_the_restatement_on_hostile_records(hipmod, w, h):
    for share, threshold in ((0.01, 0.05), (0.05, 0.3), (1.0, 0.05), (0.02, 0.0), (0.02, float("inf"))):
        m = hostile_image(w, h, 11 * w + h, share)
        for radius in RADII:
            for batch, cap in ((8, 64), (1, 2)):
                got = hipmod.adaptive_window_host(m, threshold, batch, cap, radius)
                want = awr.select(m, threshold, batch, cap, radius)
                assert np.array_equal(got.astype(bool), want), (w, h, share, threshold, radius, batch, cap, int((got.astype(bool) != want).sum()))
        sparse = awr.select(m, threshold, 8, 64, 1)
        if share < 1 and np.isfinite(threshold):
            assert 0 < sparse.sum() < w * h                                  # the case is neither empty nor saturated


@pytest.mark.parametrize("w,h", SIZES)
def test_radius_0_is_the_per_pixel_rule(hipmod, w, h):
    m = hostile_image(w, h, 5, 0.5)
    for threshold in (0.0, 0.3):
        flags, _ = hipmod.adaptive_select_host(m, threshold, 8, 64)
        assert np.array_equal(hipmod.adaptive_window_host(m, threshold, 8, 64, 0), flags)
        assert np.array_equal(awr.select(m, threshold, 8, 64, 0), aref.select(m, threshold, 8, 64))


def test_host_window_on_the_oracles_records(hipmod, veach_bank):
    for n in (8, 24):
        m = veach_bank.moments(n)
        for radius in RADII:
            got = hipmod.adaptive_window_host(m, 0.3, 8, 64, radius)
            assert np.array_equal(got.astype(bool), awr.select(m, 0.3, 8, 64, radius)), (n, radius)
    sel = [int(hipmod.adaptive_window_host(veach_bank.moments(8), 0.3, 8, 64, r).sum()) for r in RADII]
    print("VeachMIS after 8 samples, selected per radius", dict(zip(RADII, sel)))
    assert all(a < b for a, b in zip(sel, sel[1:])) and sel[-1] == 7000        # each radius adds pixels; at 8 every pixel is selected


def noisy():
    return np.array([4.0, 16.0, 2.0, 4.0], F)          # two samples 0 and 4: rel = 1 / 1.01, above every threshold used here


@pytest.mark.parametrize("radius", [1, 2, 3, 8])
def test_the_window_is_clipped_to_the_tile(hipmod, radius):
    """130 x 67: a noisy pixel in the corner (63, 63) of tile (0, 0) selects the square around it clipped to that tile and nothing in the three tiles that
    touch the corner; one just across the edge, at (64, 10), selects nothing on this side"""
    w, h = 130, 67
    m = quiet(h, w)
    m[63, 63] = noisy()
    got = hipmod.adaptive_window_host(m, 0.3, 8, 64, radius).astype(bool)
    want = np.zeros((h, w), bool)
    want[63 - radius:64, 63 - radius:64] = True
    assert np.array_equal(got, want) and np.array_equal(awr.select(m, 0.3, 8, 64, radius), want)
    m = quiet(h, w)
    m[10, 64] = noisy()
    got = hipmod.adaptive_window_host(m, 0.3, 8, 64, radius).astype(bool)
    want = np.zeros((h, w), bool)
    want[max(0, 10 - radius):10 + radius + 1, 64:64 + radius + 1] = True
    assert not got[:, :64].any() and np.array_equal(got, want)
    m = quiet(h, w)                                     # the last tile is 2 wide and 3 tall: the window stops at the image
    m[66, 129] = noisy()
    got = hipmod.adaptive_window_host(m, 0.3, 8, 64, radius).astype(bool)
    want = np.zeros((h, w), bool)
    want[max(64, 66 - radius):67, max(128, 129 - radius):130] = True
    assert np.array_equal(got, want)


def test_the_cap_is_applied_after_the_window(hipmod):
    """a noisy pixel at the cap is never selected, yet keeps its neighbours selected; a quiet neighbour at the cap is not selected either"""
    m = quiet(70, 100, 16)
    m[30, 40] = np.array([64.0, 1000.0, 64.0, 9.0], F)              # noisy, and 64 + 8 > 64
    m[30, 41, :] = quiet(1, 1, 64)[0, 0]                             # quiet, at the cap
    assert awr.above(m[30, 40], 0.3) and not awr.fits(m[30, 40], 8, 64)
    got = hipmod.adaptive_window_host(m, 0.3, 8, 64, 1).astype(bool)
    want = np.zeros((70, 100), bool)
    want[29:32, 39:42] = True
    want[30, 40] = want[30, 41] = False
    assert np.array_equal(got, want)
    assert not hipmod.adaptive_window_host(m, 0.3, 8, 64, 0).any()


@pytest.mark.parametrize("w,h", [(130, 67), (200, 130)])
def test_the_mask_does_not_depend_on_the_partition(hipmod, w, h):
    """every rank computes the rule from ITS pixels alone (the others' records are zeros to it, which are above): the union over the ranks is the one-rank mask"""
    m = hostile_image(w, h, 3, 0.03)
    for radius in (1, 3, 8):
        whole = hipmod.adaptive_window_host(m, 0.3, 8, 64, radius).astype(bool)
        for world in (1, 2, 3):
            union = np.zeros((h, w), bool)
            for rank in range(world):
                own = awr.owned(w, h, rank, world)
                xy = hipmod.tile_order(w, h, rank, world)
                assert own.sum() == len(xy) and own[xy >> 16, xy & 0xFFFF].all()
                mine = hipmod.adaptive_window_host(np.where(own[..., None], m, F(0)), 0.3, 8, 64, radius).astype(bool) & own
                assert np.array_equal(mine, whole & own), (radius, world, rank)
                union |= mine
            assert np.array_equal(union, whole)


@pytest.fixture(scope="module")
def veach_bank(oracle, rpt, world):
    return ref.SampleBank(oracle, rpt.default_config(100, 70, nee=1), world("VeachMIS"), rpt.blue_noise_seeds(100, 70))


def test_the_simulation_with_radius_0_is_the_per_pixel_simulation(veach_bank):
    for t in (aref.Target(0.3, 0, 8, 8, 64), aref.Target(0.3, 350, 8, 8, 64), aref.Target(0.2, 0, 16, 8, 40)):
        a, b = awr.simulate(veach_bank, t, 0), aref.simulate(veach_bank, t)
        assert np.array_equal(a["counts_image"], b["counts_image"])
        assert all(a[k] == b[k] for k in ("passes", "converged", "counts", "pixel_samples"))


def test_a_window_only_adds_samples(veach_bank):
    """radius 1 against radius 0 on the oracle's samples: no pixel gets fewer samples, some get more, and a pixel below the threshold is selected again — the
    closed form of the per-pixel rule does not hold"""
    t = aref.Target(0.3, 0, 8, 8, 64)
    n0, sim = aref.simulate(veach_bank, t)["counts_image"], awr.simulate(veach_bank, t, 1)
    n1 = sim["counts_image"]
    print(f"radius 1: {sim['passes']} passes, {sim['pixel_samples']} pixel-samples, per pass {sim['selected_per_pass']}")
    assert (n1 >= n0).all() and (n1 > n0).any() and not np.array_equal(n1, aref.closed_form(veach_bank, t))
    assert sim["pixel_samples"] == int(n1.sum()) and set(np.unique(n1)) <= set(aref.schedule(8, 8, 64))


def test_the_hook_refuses_what_it_cannot_compute(hipmod):
    m = quiet(23, 37)
    for bad in (dict(threshold=-1.0), dict(threshold=float("nan")), dict(radius=9), dict(radius=1 << 31)):
        args = dict(dict(threshold=0.3, radius=1), **bad)
        with pytest.raises(hipmod.RptError) as e:
            hipmod.adaptive_window_host(m, args["threshold"], 8, 64, args["radius"])
        assert e.value.code == -1, bad
    L = hipmod.lib()
    flags = np.zeros((23, 37), np.uint8)
    assert L.rpt_debug_adaptive_window_host(None, 37, 23, 0.3, 8, 64, 1, hipmod.ptr(flags)) == -1
    assert L.rpt_debug_adaptive_window_host(hipmod.ptr(m), 37, 23, 0.3, 8, 64, 1, None) == -1
    assert L.rpt_debug_adaptive_window_host(hipmod.ptr(m), 0, 23, 0.3, 8, 64, 1, hipmod.ptr(flags)) == -1
    assert L.rpt_debug_adaptive_window_host(hipmod.ptr(m), 37, 65536, 0.3, 8, 64, 1, hipmod.ptr(flags)) == -1
    assert not flags.any()
    assert hipmod.adaptive_window_host(m, 0.3, 8, 64, 8).sum() == 0 and hipmod.ADAPTIVE_MAX_RADIUS == 8


def test_the_recommended_radius_is_the_minimum_of_the_kept_grid(hipmod):
    """profiles/r17_adaptive_window_quality.txt (tools/adaptive_probe.py --cpu-window): hip.ADAPTIVE_WINDOW_RADIUS is the radius with the lowest summed rel-L2 of
    its first grid, over the three configurations the file names; radius 0, the per-pixel rule, is in the grid and is not the minimum"""
    text = open(os.path.join(ROOT, "profiles", "r17_adaptive_window_quality.txt")).read()
    assert all(s in text for s in ("DarkCornell/nee0", "DarkCornell/nee1", "VeachMIS/nee1", "energy", "uniform"))
    lines = text.splitlines()
    head = next(k for k, l in enumerate(lines) if l.startswith("grid 100 x 70"))
    rows = [[float(v) for v in l.split("|")] for l in lines[head + 1:head + 5]]
    assert [r[0] for r in rows] == [0, 1, 2, 3]
    best = min(rows, key=lambda r: r[1])
    assert best[0] == hipmod.ADAPTIVE_WINDOW_RADIUS != 0 and 1 <= hipmod.ADAPTIVE_WINDOW_RADIUS <= hipmod.ADAPTIVE_MAX_RADIUS
    assert len(re.findall(r"^  radius \d:", text, flags=re.M)) >= 12
