"""The noise estimate of csrc/k_moments.h without a GPU: the host build of noise_rel inside librpt_hip.so (rpt_debug_noise_host) against the numpy
restatement of tests/moments_ref.py — bit for bit on rel, equal on the counts — and the null-pointer contract of the new entry points."""
import ctypes as C

import numpy as np
import pytest

import moments_ref as ref

F = np.float32
THRESHOLDS = (0.0, 0.3, float("inf"))


def check(hipmod, m):
    m = np.ascontiguousarray(m, F).reshape(-1, 4)
    want = ref.noise_rel(m)
    for t in THRESHOLDS:
        rel, counts = hipmod.noise_host(m, t)
        assert ref.same_bits(rel, want), np.flatnonzero(rel.view(np.uint32) != want.view(np.uint32))[:8]
        assert counts == ref.noise_counts(m, t), t
    return want


def test_noise_host_equals_the_numpy_restatement_on_random_records(hipmod):
    """10^5 records as a render leaves them: n samples of non-negative luminance, accumulated by the restatement of mo_add in f32 — a third of them with
    few samples, a third with a firefly among them, a third as they come"""
    rng = np.random.default_rng(20261018)
    N = 100_000
    m = np.zeros((N, 4), F)
    n = rng.integers(0, 40, N)
    n[: N // 3] = rng.integers(0, 4, N // 3)
    scale = np.exp(rng.uniform(-12, 6, N)).astype(F)
    for k in range(int(n.max())):
        y = (rng.random(N).astype(F) ** 3) * scale
        if k == 2:
            y[N // 3: 2 * N // 3] *= F(1e4)
        live = k < n
        r = np.stack([y, y, y], axis=-1)
        m[live] = ref.add_sample(m[live], r[live])
    assert np.array_equal(m[:, 2], n.astype(F))
    rel = check(hipmod, m)
    measured = n >= 2
    assert np.all(np.isinf(rel[~measured])) and np.all(np.isfinite(rel[measured])) and (rel[measured] > 0).sum() > 50_000


def test_noise_host_equals_the_numpy_restatement_on_random_bits(hipmod):
    """10^5 records of arbitrary finite sums, either sign, with sample counts from 0 to 2^24"""
    rng = np.random.default_rng(7)
    N = 100_000
    m = np.zeros((N, 4), F)
    m[:, 0] = (rng.standard_normal(N) * np.exp(rng.uniform(-30, 30, N))).astype(F)
    m[:, 1] = (np.abs(rng.standard_normal(N)) * np.exp(rng.uniform(-40, 60, N))).astype(F)
    m[:, 2] = rng.choice([0, 1, 2, 3, 8, 31, 1000, 2 ** 24], N).astype(F)
    m[:, 3] = rng.standard_normal(N).astype(F)
    check(hipmod, m)


def test_noise_host_on_hostile_records(hipmod):
    inf, nan, big = F(np.inf), F(np.nan), F(3e38)
    rows = []
    for n in (0, 1, 2, 2 ** 24):
        rows += [(0, 0, n, 0), (4, 9, n, 3), (-4, 9, n, 1), (1e-30, 1e-38, n, 1e-30)]
    rows += [(inf, 1, 8, 1), (1, inf, 8, 1), (-inf, inf, 8, 1), (nan, 1, 8, 1), (1, nan, 8, 1), (nan, nan, 2, nan), (inf, inf, 1, inf)]     # sums that are not finite
    rows += [(8, 7.9999995, 8, 1), (3, 2.9999998, 3, 1), (0.3, 0.03, 3, 0.1), (1e19, 1e37, 10, 1e19)]      # m.y < m.x^2 / n: ss negative from rounding
    rows += [(8, 8, 8, 1), (2, 2, 2, 1), (0.5, 0.125, 2, 0.25), (0, 0, 100, 0)]                            # zero variance
    rows += [(-8, 40, 8, 0), (-1e-3, 1e-3, 4, 0), (-0.02, 0.5, 2, 0)]                                      # negative mean (|mean| in the denominator)
    rows += [(big, big, 2, big), (big, 1, 2, 1), (1, big, 2 ** 24, 1), (1e-45, 1e-45, 2, 1e-45)]           # overflow of m.x * m.x, denormals
    m = np.array(rows, F)
    rel = check(hipmod, m)
    by = {tuple(r): v for r, v in zip(rows, rel)}
    assert all(np.isinf(v) and v > 0 for r, v in by.items() if r[2] < 2)
    assert all(np.isinf(by[r]) for r in rows if not (np.isfinite(F(r[0])) and np.isfinite(F(r[1]))))
    assert by[(8, 8, 8, 1)] == 0 and by[(8, 7.9999995, 8, 1)] == 0 and by[(0, 0, 100, 0)] == 0           # never a NaN from a negative ss
    assert by[(-8, 40, 8, 0)] > 0 and np.isfinite(by[(-8, 40, 8, 0)])
    # the counts by hand for one threshold: measured = n >= 2; above = measured and not (rel <= 0.3), so an infinite rel of a measured record counts
    _, counts = hipmod.noise_host(m, 0.3)
    measured = m[:, 2] >= 2
    assert counts["pixels"] == len(m) and counts["measured"] == measured.sum() and counts["above"] == (measured & ~(rel <= F(0.3))).sum()
    assert hipmod.noise_host(m, float("inf"))[1]["above"] == 0 and hipmod.noise_host(np.zeros((0, 4), F))[1] == {"pixels": 0, "measured": 0, "above": 0}


def test_noise_host_refuses_a_bad_threshold(hipmod):
    for t in (-0.5, float("nan")):
        with pytest.raises(hipmod.RptError) as e:
            hipmod.noise_host(np.zeros((4, 4), F), t)
        assert e.value.code == -1


def test_null_pointers_are_refused_without_a_device(hipmod):
    L = hipmod.lib()
    on, counts, target, result = C.c_uint32(), hipmod.NoiseCounts(), hipmod.NoiseTarget(0.1, 8, 64, 8, 0), hipmod.NoiseResult()
    buf = np.zeros(16, F)
    p = hipmod.ptr(buf)
    assert L.rpt_set_moments(None, 1) == -1 and L.rpt_moments(None, C.byref(on)) == -1
    assert L.rpt_read_moments(None, p) == -1 and L.rpt_read_noise(None, p) == -1
    assert L.rpt_noise_count(None, 0.1, C.byref(counts)) == -1
    assert L.rpt_render_to_noise(None, C.byref(target), C.byref(result)) == -1
    assert L.rpt_multi_set_moments(None, 1) == -1 and L.rpt_multi_read_moments(None, p) == -1
    assert L.rpt_multi_noise_count(None, 0.1, C.byref(counts)) == -1
    assert L.rpt_multi_render_to_noise(None, C.byref(target), C.byref(result)) == -1
    assert L.rpt_debug_noise_host(None, 4, 0.1, p, C.byref(counts)) == -1
