"""The selection rule and the pass schedule of rpt_render_adaptive without a GPU: the host build of csrc/k_adaptive.h (rpt_debug_adaptive_select_host) against the
numpy restatement of tests/adaptive_ref.py, and the documented closed form of a pixel's final count against the pass-by-pass simulation, on the CPU oracle's
samples."""
import numpy as np
import pytest

import adaptive_ref as aref
import moments_ref as ref

F = np.float32


def hostile_records(n, seed):
    """moments records (sum Y, sum Y^2, n, max Y): plausible ones, and ones with NaN / inf sums, counts of 0, 1 and 2, counts next to the cap, zero variance"""
    g = np.random.default_rng(seed)
    count = g.integers(0, 70, n).astype(F)
    mean = g.gamma(0.5, 2.0, n).astype(F)
    spread = (g.random(n) ** 4).astype(F) * F(3)
    m = np.zeros((n, 4), F)
    m[:, 0] = mean * count
    m[:, 1] = (mean * mean * (F(1) + spread)) * count
    m[:, 2] = count
    m[:, 3] = mean * F(2)
    kind = g.integers(0, 16, n)
    m[kind == 0, 0] = np.nan
    m[kind == 1, 1] = np.inf
    m[kind == 2, 0] = -np.inf
    m[kind == 3, 2] = g.integers(0, 3, (kind == 3).sum()).astype(F)          # n of 0, 1 and 2
    m[kind == 4, 1] = m[kind == 4, 0] * m[kind == 4, 0] / np.maximum(m[kind == 4, 2], F(1))   # zero (or rounding-negative) variance
    m[kind == 5, 2] = np.nan
    m[kind == 6, :2] = 0                                                    # a black pixel
    return m


@pytest.mark.parametrize("threshold", [0.0, 0.05, 0.3, float("inf")])
def test_host_selection_is_the_restatement(hipmod, threshold):
    m = hostile_records(100_000, 7)
    for batch, cap in ((8, 64), (1, 2), (16, 16), (8, 4), (3, 70)):
        flags, active = hipmod.adaptive_select_host(m, threshold, batch, cap)
        want = aref.select(m, threshold, batch, cap)
        assert np.array_equal(flags.astype(bool), want), (threshold, batch, cap)
        assert np.array_equal(active, aref.compact(want)) and np.all(np.diff(active.astype(np.int64)) > 0)
    flags, _ = hipmod.adaptive_select_host(m, threshold, 8, 64)
    unmeasured = m[:, 2] < 2
    if np.isfinite(threshold):
        assert flags[unmeasured & (m[:, 2] + 8 <= 64)].all()            # an unmeasured pixel is selected while the batch fits
        assert flags[np.isnan(m[:, 0]) & (m[:, 2] + 8 <= 64)].all()     # and so is one whose sums are not finite
    assert not flags[np.isnan(m[:, 2])].any()                           # a NaN count fits under no cap
    assert 0 < flags.sum() < len(m) or not np.isfinite(threshold)


def test_host_selection_refuses_bad_thresholds(hipmod):
    m = hostile_records(16, 1)
    for t in (-1.0, float("nan")):
        with pytest.raises(hipmod.RptError) as e:
            hipmod.adaptive_select_host(m, t, 8, 64)
        assert e.value.code == -1
    flags, active = hipmod.adaptive_select_host(np.zeros((0, 4), F), 0.3, 8, 64)
    assert flags.size == 0 and active.size == 0


@pytest.fixture(scope="module")
def veach_bank(oracle, rpt, world):
    return ref.SampleBank(oracle, rpt.default_config(100, 70, nee=1), world("VeachMIS"), rpt.blue_noise_seeds(100, 70))


@pytest.mark.parametrize("threshold,batch,cap", [(0.3, 8, 64), (0.2, 8, 40), (0.3, 16, 60), (0.05, 8, 24)])
def test_closed_form_is_the_simulation(veach_bank, threshold, batch, cap):
    """max_above = 0: a pixel stops at the first count of the schedule at which its noise is at or below the threshold, or at the last count that fits"""
    t = aref.Target(threshold, 0, batch, 8, cap)
    sim = aref.simulate(veach_bank, t)
    steps = aref.schedule(8, batch, cap)
    assert np.array_equal(sim["counts_image"], aref.closed_form(veach_bank, t))
    assert set(np.unique(sim["counts_image"])) <= set(steps)
    assert sim["passes"] == (int(sim["counts_image"].max()) - 8) // batch
    assert sim["pixel_samples"] == int(sim["counts_image"].sum())
    at_cap = sim["counts_image"] == steps[-1]
    assert sim["converged"] == int(not aref.select(aref.moments_at(veach_bank, sim["counts_image"]), threshold, 0, 1 << 20)[at_cap].any())


def test_expected_state_of_a_uniform_count_is_the_bank(veach_bank):
    acc, rng, mom = aref.expected_state(veach_bank, np.full((70, 100), 5))
    assert ref.same_bits(acc, veach_bank.accum(5)) and ref.same_bits(mom, veach_bank.moments(5))
    assert np.array_equal(rng.reshape(-1), np.asarray(veach_bank.rng(5)).reshape(-1))
    acc, rng, mom = aref.expected_state(veach_bank, np.zeros((70, 100), int))
    assert not acc.any() and not mom.any() and np.array_equal(rng.reshape(-1), np.asarray(veach_bank.rng(0)).reshape(-1))
