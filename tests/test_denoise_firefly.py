"""The firefly clamp without a GPU: the host build of csrc/k_firefly.h ff_pixel (hipmod.firefly_host, and the variance and temporal host hooks with the clamp
fields set) against the numpy restatement of tests/firefly_ref.py, bit for bit; the rule's properties; an independent float64 restatement; the refusals; the
shipped defaults against the kept grid; and the count of clamped pixels on the oracle's DarkCornell."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_ref
import firefly_ref
import moments_ref
from conftest import ROOT
from test_denoise_temporal import MOVED, camera, previous_of, records, room
from test_denoise_variance import assert_same_bits, guides_for, image_and_moments

F = np.float32
SIZES = [(37, 23), (130, 67)]                          # more than two 64-pixel segments per row, heights that are no multiple of 4
N = 8


def planted(w, h, seed, n=N, spikes=0.03, gain=1.0):
    """records accumulated by moments_ref.add_sample from n gamma-distributed samples per pixel, a few pixels with one sample 20 to 200 times `gain` brighter; the mean"""
    rng = np.random.default_rng(seed)
    level = (0.05 + rng.random((h, w, 1))).astype(F)
    m, sums = np.zeros((h, w, 4), F), np.zeros((h, w, 3), F)
    spike = rng.random((h, w)) < spikes
    when = rng.integers(0, n, (h, w))
    for k in range(n):
        s = (rng.gamma(2.0, 0.3, (h, w, 3)).astype(F) * level).astype(F)
        hot = spike & (when == k)
        s[hot] = (s[hot] * rng.uniform(20 * gain, 200 * gain, (int(hot.sum()), 1))).astype(F)
        moments_ref.add_sample(m, s)
        sums = (sums + s).astype(F)
    return (sums / F(n)).astype(F), m, spike


def hostile(w, h, seed):
    """planted(), with records of every awkward sort strewn in, a block of unsampled records (windows without an eligible tap), lone pixels of their kind, and
    in a patch of calm records one record each of 1, 2 and 2^24 samples (to be clamped as centres where the counts are the records' own)"""
    mean, m, spike = planted(w, h, seed)
    calm = np.where(spike[..., None], np.array([4, 3, N, 1], F), m).astype(F)
    rng = np.random.default_rng(seed + 1)
    tiny = F(1e-42)
    recs = [[np.nan, 1, N, 1], [1, np.nan, N, 1], [1, 1, np.nan, 1], [1, 1, N, np.nan], [np.inf, 1, N, 1], [1, np.inf, N, 1], [1, 1, np.inf, 1], [1, 1, N, np.inf],
            [-np.inf, 1, N, 1], [1, 1, N, -np.inf], [-3, 2, N, 1], [3, -2, N, 1], [3, 2, N, -1], [0, 0, 0, 0], [5, 25, 1, 5], [9, 60, 2, 8], [1e3, 1e2, 2.0 ** 24, 50],
            [7, 49, N, 7], [7.000001, 49, N, 7], [tiny, 0, N, tiny], [4 * tiny, 0, N, 3 * tiny], [3e38, 3e38, N, 3e38], [1e20, 3e38, N, 1e20], [40, 900, N, 30], [400, 90000, N, 300]]
    recs = np.array(recs, F)
    bad = rng.random((h, w)) < 0.15
    m[bad] = recs[rng.integers(0, len(recs), int(bad.sum()))]
    m[2:9, 3:10] = 0                                   # unsampled: the pixel in the middle has no eligible tap at any radius
    m[5, 6] = [40, 900, N, 30]
    m[h - 11:h - 4, 2:23] = calm[h - 11:h - 4, 2:23]
    m[h - 8, 5], m[h - 8, 12], m[h - 8, 19] = [5, 25, 1, 5], [9, 60, 2, 8], [1e3, 1e2, 2.0 ** 24, 50]
    return mean, m


def guides(w, h, seed):
    g = guides_for(w, h, seed)
    g["kind"][2:9, 3:10] = g["kind"][5, 6]
    g["kind"][h - 4, w - 5] = 7                        # a lone pixel of its kind
    return g


def run(hipmod, mean, g, m, counts, scale, floor, radius, dem):
    uniform = np.ndim(counts) == 0
    return hipmod.firefly_host(mean, g["albedo"], g["kind"], m, None if uniform else counts, int(counts) if uniform else 0, scale, floor, radius, dem)


def assert_clamp_same(got, want, what):
    assert_same_bits(got[0], want[0], what + ": c'")
    assert_same_bits(got[1], want[1], what + ": m'")
    assert np.array_equal(got[2] != 0, want[2]), what + ": mask"


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("dem", [False, True])
def test_host_hook_equals_the_numpy_restatement_bitwise(hipmod, w, h, radius, dem):
    g = guides(w, h, 31 * w + h)
    clamped = 0
    centres = {1.0: 0, 2.0: 0, 2.0 ** 24: 0}            # hostile records of 1, 2 and 2^24 samples that were clamped as CENTRES (counts == m.z)
    for name, (mean, m) in (("planted", planted(w, h, w + radius)[:2]), ("hostile", hostile(w, h, h + radius))):
        own = np.where(np.random.default_rng(5).random((h, w)) < 0.2, F(N + 5), F(N)).astype(F)            # per-pixel counts: a fifth of the pixels count differently
        for label, counts in (("uniform", N), ("own", own), ("the records'", m[..., 2].copy())):
            for scale, floor in ((1.0, 0.0), (2.0, 0.0), (0.5, 0.4), (8.0, 0.0)):
                what = f"{w}x{h} {name} radius {radius} demodulated {dem} scale {scale} floor {floor} counts {label}"
                got = run(hipmod, mean, g, m, counts, scale, floor, radius, dem)
                want = firefly_ref.clamp(mean, g["albedo"], g["kind"], m, counts, scale, floor, radius, dem)
                assert_clamp_same(got, want, what)
                clamped += int(want[2].sum())
                if label == "the records'":
                    for n in centres:
                        centres[n] += int((want[2] & (m[..., 2] == F(n))).sum())
                assert not want[2][np.broadcast_to(np.asarray(counts, F), (h, w)) != m[..., 2]].any(), what     # m.z != count: left alone
    assert clamped > 0 and all(v > 0 for v in centres.values()), centres
    # the unsampled block's middle pixel and the lone pixel of its kind have no eligible tap: never clamped, whatever the scale
    mean, m = hostile(w, h, 1)
    m[h - 4, w - 5] = [400, 90000, N, 300]
    got = run(hipmod, mean, g, m, N, 0.001, 0.0, radius, dem)
    assert got[2][5, 6] == 0 and got[2][h - 4, w - 5] == 0 and got[2].sum() > 0
    assert_same_bits(got[1][5, 6], m[5, 6], "no eligible tap")
    assert_same_bits(got[0][5, 6], mean[5, 6], "no eligible tap")


@pytest.mark.parametrize("w,h", SIZES)
def test_properties_of_the_rule(hipmod, w, h):
    g = guides(w, h, 3)
    mean, m, spike = planted(w, h, 11)
    for radius, dem in ((1, False), (2, True), (3, False)):
        c1, m1, mask = run(hipmod, mean, g, m, N, 2.0, 0.0, radius, dem)
        mask = mask != 0
        assert mask.any() and (dem or (mask & spike).sum() > 0.5 * mask.sum())       # it finds the planted spikes (the synthetic radiance does not scale with the albedo)
        assert (c1 <= mean).all() and (c1[mask] < mean[mask]).any()                     # c' <= c per channel for c >= 0
        assert (m1[mask][:, 3] < m[mask][:, 3]).all()                                   # m'.w == L < m.w exactly on the mask ...
        assert_same_bits(m1[~mask], m[~mask], "records off the mask")
        assert_same_bits(c1[~mask], mean[~mask], "means off the mask")
        assert_same_bits(m1[mask][:, 3], firefly_ref.limit(g["albedo"], g["kind"], m, 2.0, 0.0, radius, dem)[1][mask], "m'.w == L")    # ... and it is the limit, bit for bit
        assert (m1[mask][:, 2] == N).all() and (m1[..., :2] >= 0).all()
    # m.z != count leaves a pixel alone: the same image, counted as N + 1 everywhere
    assert run(hipmod, mean, g, m, N + 1, 2.0, 0.0, 2, False)[2].sum() == 0
    assert run(hipmod, mean, g, m, np.full((h, w), F(N + 1)), 2.0, 0.0, 2, False)[2].sum() == 0


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_the_window_its_corners_the_borders_and_the_kinds(hipmod, radius):
    """a flat image (every record's brightest sample 1) with one centre of 10: a second spike of 10 shields it from a corner of the window and not from one
    pixel further out; at the image's borders; and not when it is of another kind"""
    w, h = 23, 17
    flat = np.tile(np.array([4, 3, N, 1], F), (h, w, 1))
    mean = np.full((h, w, 3), F(0.5))
    one = {"albedo": np.ones((h, w, 3), F), "kind": np.ones((h, w), np.uint32)}
    for cy, cx in ((8, 11), (0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0)):
        m = flat.copy()
        m[cy, cx] = [13, 103, N, 10]
        c1, m1, mask = run(hipmod, mean, one, m, N, 2.0, 0.0, radius, False)
        assert mask.sum() == 1 and mask[cy, cx] == 1 and m1[cy, cx, 3] == 2.0 and m1[cy, cx, 0] == 5.0 and m1[cy, cx, 1] == 7.0
        assert_same_bits(c1[cy, cx], (mean[cy, cx] * (F(5.0) / F(13.0))).astype(F), "rho")
        for sy in (-1, 1):
            for sx in (-1, 1):
                for d, shielded in ((radius, True), (radius + 1, False)):
                    qy, qx = cy + sy * d, cx + sx * d
                    if not (0 <= qy < h and 0 <= qx < w):
                        continue
                    m2 = m.copy()
                    m2[qy, qx] = [13, 103, N, 10]
                    got = run(hipmod, mean, one, m2, N, 2.0, 0.0, radius, False)[2]
                    assert (got[cy, cx] == 0) == shielded, (radius, cy, cx, qy, qx)
                    if shielded:                                                        # a spike of another kind does not shield
                        k2 = {"albedo": one["albedo"], "kind": one["kind"].copy()}
                        k2["kind"][qy, qx] = 2
                        assert run(hipmod, mean, k2, m2, N, 2.0, 0.0, radius, False)[2][cy, cx] == 1


@pytest.mark.parametrize("dem", [False, True])
def test_records_of_one_two_and_2_24_samples_as_centres(hipmod, dem):
    """a flat image with centres of n = 1 (m.x == m.w, so x' == L and rho == L / m.x), 2 and 2^24 samples, counted by a counts image equal to m.z: by hand
    where not demodulated, and against numpy"""
    w, h = 23, 17
    m = np.tile(np.array([4, 3, N, 1], F), (h, w, 1))
    m[4, 5], m[8, 11], m[12, 17] = [5, 25, 1, 5], [9, 68, 2, 8], [1e4, 2.6e7, 2.0 ** 24, 5000]
    mean = np.full((h, w, 3), F(0.5))
    g = guides_for(w, h, 2)
    g = {"albedo": g["albedo"] if dem else np.ones((h, w, 3), F), "kind": np.ones((h, w), np.uint32)}
    counts = m[..., 2].copy()
    got = run(hipmod, mean, g, m, counts, 2.0, 0.0, 2, dem)
    assert_clamp_same(got, firefly_ref.clamp(mean, g["albedo"], g["kind"], m, counts, 2.0, 0.0, 2, dem), f"demodulated {dem}")
    L = firefly_ref.limit(g["albedo"], g["kind"], m, 2.0, 0.0, 2, dem)[1]
    for at in ((4, 5), (8, 11), (12, 17)):
        assert got[2][at] == 1 and got[1][at][2] == m[at][2] and got[1][at][3] == L[at] < m[at][3], at
    assert got[1][4, 5, 0] == L[4, 5] and np.array_equal(got[0][4, 5], (mean[4, 5] * (L[4, 5] / F(5.0))).astype(F))      # n == 1: x' == (5 - 5) + L
    if not dem:
        assert got[1][4, 5].tolist() == [2.0, 4.0, 1.0, 2.0] and got[1][8, 11].tolist() == [3.0, 8.0, 2.0, 2.0] and got[1][12, 17].tolist() == [5002.0, 1000004.0, 2.0 ** 24, 2.0]
    assert run(hipmod, mean, g, m, N, 2.0, 0.0, 2, dem)[2][[4, 8, 12], [5, 11, 17]].sum() == 0          # counted as N everywhere: left alone


@pytest.mark.parametrize("radius", [1, 2, 3])
def test_scale_one_on_distinct_maxima_clamps_exactly_the_strict_local_maxima(hipmod, radius):
    w, h = 37, 23
    rng = np.random.default_rng(radius)
    top = rng.permutation(w * h).reshape(h, w).astype(F) + F(1.0)                       # distinct brightest samples
    m = np.stack([top * 2, top * top * 2, np.full((h, w), F(N)), top], -1).astype(F)
    one = {"albedo": np.ones((h, w, 3), F), "kind": np.ones((h, w), np.uint32)}
    mask = run(hipmod, np.ones((h, w, 3), F), one, m, N, 1.0, 0.0, radius, False)[2]
    pad = np.pad(top, radius, constant_values=-1.0)
    local = np.ones((h, w), bool)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            if (dy, dx) != (radius, radius):
                local &= top > pad[dy:dy + h, dx:dx + w]
    assert np.array_equal(mask != 0, local) and 0 < local.sum() < w * h // (radius + 1) ** 2


def garbage(p):
    """the clamp's second and third word set to bit patterns no parameter check would pass"""
    q = type(p)()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    f = q.filter if hasattr(q, "filter") else q
    f.clamp_floor, f.clamp_radius = float("nan"), 0xDEADBEEF
    return q


@pytest.mark.parametrize("w,h", SIZES)
def test_the_variance_hook_with_the_clamp(hipmod, oracle, w, h):
    g = guides(w, h, w)
    args = lambda mean, m, p, op: (mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], m, p, op)
    for k, (mean, m) in enumerate((planted(w, h, 3)[:2], image_and_moments(w, h, 4, True))):
        for it, dem, radius in ((2, 1, 2), (1, 0, 3), (0, 1, 1)):
            p = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_variance=4.0, clamp_scale=2.0, clamp_radius=radius, clamp_floor=0.01)
            rgb, var = hipmod.denoise_variance_host(*args(mean, m, p, it))
            want = firefly_ref.denoise_variance(mean, g, m, p, it, oracle)
            what = f"{w}x{h} inputs {k} iterations {it} demodulate {dem} radius {radius}"
            assert_same_bits(rgb, want[0], what + ": colour")
            assert_same_bits(var, want[1], what + ": variance")
            assert want[2].any(), what
            off = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_variance=4.0)
            a, b = hipmod.denoise_variance_host(*args(mean, m, off, it)), hipmod.denoise_variance_host(*args(mean, m, garbage(off), it))
            assert off.clamp_scale == 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), what
            assert a[0].tobytes() != rgb.tobytes(), what                                 # (the clamp does something)


def test_the_temporal_hook_with_the_clamp(rpt, hipmod, oracle):
    w, h = 130, 67
    cam_a, cam_b = camera(rpt, w, h), camera(rpt, w, h, **MOVED)
    g0, g1 = room(cam_a, oracle, 1), room(cam_b, oracle, 2)
    prev = previous_of(cam_a, g0, records(w, h, 5, False))
    run_t = lambda mean, m, previous, p: hipmod.denoise_temporal_host(mean, g1["albedo"], g1["normal"], g1["position"], g1["depth"], g1["kind"], m, cam_b, previous, p, 0)
    for k, (mean, m) in enumerate((planted(w, h, 8)[:2], image_and_moments(w, h, 9, True))):
        for it, dem, radius, previous in ((2, 1, 2, prev), (1, 0, 1, prev), (2, 1, 3, None)):
            p = hipmod.temporal_params(iterations=it, demodulate=dem, sigma_variance=4.0, max_history=16.0, clamp_scale=2.0, clamp_radius=radius)
            got = run_t(mean, m, previous, p)
            want = firefly_ref.denoise_temporal(mean, g1, m, cam_b, previous, p, 0, oracle)
            what = f"inputs {k} iterations {it} demodulate {dem} radius {radius}"
            for key in ("rgb", "variance", "history", "records"):
                assert_same_bits(got[key], want[key], f"{what}: {key}")
            assert got["pixels_with_history"] == want["pixels_with_history"] and want["mask"].any(), what
            off = hipmod.temporal_params(iterations=it, demodulate=dem, sigma_variance=4.0, max_history=16.0)
            a, b = run_t(mean, m, previous, off), run_t(mean, m, previous, garbage(off))
            assert all(a[key].tobytes() == b[key].tobytes() for key in ("rgb", "variance", "history", "records")), what
            # a clamped pixel without history keeps c' (in the filter's units), not c, as its history
            if k == 0 and not dem:
                fresh = want["mask"] & (got["history"] == m[..., 2])
                c1 = firefly_ref.clamp(mean, g1["albedo"], g1["kind"], m, m[..., 2], 2.0, 0.0, radius, False)[0]
                assert fresh.any() and np.array_equal(got["records"][fresh][:, :3], c1[fresh]) and not np.array_equal(c1[fresh], mean[fresh])


def test_refusals(rpt, hipmod):
    w, h = 8, 6
    g = guides_for(w, h, 1)
    mean, m, _ = planted(w, h, 1)
    bad = [dict(clamp_scale=-1.0), dict(clamp_scale=float("nan")), dict(clamp_scale=float("inf")), dict(clamp_scale=1.0, clamp_floor=-0.5),
           dict(clamp_scale=1.0, clamp_floor=float("nan")), dict(clamp_scale=1.0, clamp_floor=float("inf")), dict(clamp_scale=1.0, clamp_radius=0),
           dict(clamp_scale=1.0, clamp_radius=4)]
    for fields in bad:
        with pytest.raises(hipmod.RptError) as e:
            hipmod.denoise_variance_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], m, hipmod.denoise_var_params(**fields), 0)
        assert e.value.code == -1 and "clamp" in str(e.value), fields
        with pytest.raises(hipmod.RptError):
            hipmod.denoise_temporal_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], m, rpt.default_config(w, h), None,
                                         hipmod.temporal_params(**fields), 0)
        f = dict(dict(clamp_scale=1.0, clamp_floor=0.0, clamp_radius=2), **fields)
        with pytest.raises(hipmod.RptError):
            hipmod.firefly_host(mean, g["albedo"], g["kind"], m, None, N, f["clamp_scale"], f["clamp_floor"], f["clamp_radius"], True)
    # while the clamp is off the other two words are not read
    hipmod.denoise_variance_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], m, hipmod.denoise_var_params(clamp_floor=-1.0, clamp_radius=99), 0)
    off = hipmod.firefly_host(mean, g["albedo"], g["kind"], m, None, N, 0.0, -1.0, 0, True)
    assert off[2].sum() == 0 and off[0].tobytes() == mean.tobytes() and off[1].tobytes() == m.tobytes()
    assert C.sizeof(hipmod.DenoiseVarParams) == 48 and C.sizeof(hipmod.TemporalParams) == 80 and C.sizeof(hipmod.DenoiseReport) == 24      # the sizes of ABI version 3


def test_the_recommended_settings_are_the_minima_of_the_kept_grid_and_the_clamp_ships_off(hipmod):
    """profiles/r16_firefly_quality.txt: the first row of the first sorted grid (rpt_denoise_variance, the shipped filter) is hip.FIREFLY_CLAMP_VARIANCE, that of
    the third (the eight-view path) hip.FIREFLY_CLAMP_TEMPORAL, and both beat the clamp off there.  Neither minimum is clamp_scale 0, and still both sets of
    defaults ship the clamp OFF: with it on a call that never asked would return other bytes than before the fields existed (rpt_denoise_variance with
    sigma_variance 0 is rpt_denoise bit for bit, and the tests of N8 and N9 say so).  The defaults carry the minima's clamp_radius, so that clamp_scale alone
    turns the recommended window on."""
    text = open(os.path.join(ROOT, "profiles", "r16_firefly_quality.txt")).read()
    assert all(s in text for s in ("DarkCornell/nee0", "DarkCornell/nee1", "VeachMIS/nee1", "PBRTest/nee0", "@1", "@2", "@4", "lost"))
    lines = text.splitlines()
    heads = [k for k, l in enumerate(lines) if l.startswith("grid (sorted")]
    assert len(heads) == 3
    for head, p, best in ((heads[0], hipmod.denoise_var_params(), hipmod.FIREFLY_CLAMP_VARIANCE), (heads[2], hipmod.temporal_params().filter, hipmod.FIREFLY_CLAMP_TEMPORAL)):
        rows = [[float(v) for v in l.split("|")[0].split()] + [float(l.split("|")[2])] for l in lines[head + 1:head + 16]]
        assert len(rows) == 15 and sorted({r[0] for r in rows}) == [0, 1, 2, 4, 8] and sorted({r[1] for r in rows}) == [1, 2, 3] and rows[0][2] == min(r[2] for r in rows)
        assert rows[0][:2] == [best["clamp_scale"], best["clamp_radius"]] and best["clamp_floor"] == 0
        assert rows[0][2] < min(r[2] for r in rows if r[0] == 0)
        assert p.clamp_scale == 0 and p.clamp_floor == 0 and p.clamp_radius == best["clamp_radius"]


def test_clamped_pixels_of_the_oracles_darkcornell(rpt, hipmod, world, oracle):
    """DarkCornell with NEE at 130 x 67, 8 spp, radius 2, scale 2, on the oracle's samples and the numpy guides: the count of clamped pixels lies in
    [1, pixels / 8] — a condition against a vacuous or runaway rule, not a measurement (67 on the CPU without the kind test, 345 at scale 1)"""
    w, h = 130, 67
    cfg = rpt.default_config(w, h, nee=1)
    bank = moments_ref.SampleBank(oracle, cfg, world("DarkCornell"), rpt.blue_noise_seeds(w, h))
    acc, m = bank.accum(8), bank.moments(8)
    g = denoise_ref.guides(world("DarkCornell"), cfg, oracle)
    mean = (acc[..., :3] / F(8)).astype(F)
    for dem in (True, False):
        got = hipmod.firefly_host(mean, g["albedo"], g["kind"], m, None, 8, 2.0, 0.0, 2, dem)
        want = firefly_ref.clamp(mean, g["albedo"], g["kind"], m, 8, 2.0, 0.0, 2, dem)
        assert_clamp_same(got, want, f"oracle, demodulated {dem}")
        count, at_one = int(got[2].sum()), int(hipmod.firefly_host(mean, g["albedo"], g["kind"], m, None, 8, 1.0, 0.0, 2, dem)[2].sum())
        lost = 1.0 - got[0].astype(np.float64).sum() / mean.astype(np.float64).sum()
        print(f"DarkCornell nee 1, 130 x 67, 8 spp, radius 2, demodulated {dem}: {count} pixels clamped at scale 2 ({100 * lost:.1f} % of the radiance removed), {at_one} at scale 1")
        assert 1 <= count <= w * h // 8 and count < at_one


# ---- float64 -------------------------------------------------------------------------------------------------------------------------------------------

U = 2.0 ** -24


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("dem", [False, True])
def test_the_rule_against_an_independent_float64_restatement(hipmod, w, h, dem):
    """firefly_ref.clamp64 on finite records with planted spikes.  The two precisions must take the same decision (w > L; the eligibility of a tap is a
    comparison of exact inputs and agrees by construction) except where |w - L| <= 4 ulp of L, and those pixels — at most 1 % — are left out.
    Rounding counts, u = 2^-24 (half an ulp, relative); S = 1 + 32 u covers the products of two roundings:
      Ya   three products and two sums of positive terms           3u          (1, exactly, where not demodulated)
      L    b = w_q / Ya_q (3u + u), scale * B (u), * Ya_p (3u + u)  e_L = 9u    (u where not demodulated: only scale * B rounds)
      x'   = (m.x - w) + L        u |m.x - w| + e_L L + u |x'|                  absolute; relative to m.x + w + L it is a few u
      rho  = x' / m.x             tol(x') / m.x + u rho
      c'   = c rho                |c| tol(rho) + u |c'|
      y'   = (m.y - w w) + L L    w w rounds (u w^2), the difference rounds (u |m.y - w^2|), L L carries L's error twice and rounds ((2 e_L + u) L^2), the
                                  sum rounds (u y'):   D = S (u w^2 + u |m.y - w^2| + (2 e_L + u) L^2 + u y').
    y' is held to TWO bounds.  Everywhere to D.  And to the bound the rule's text names, 3 u w^2, wherever its premise holds — the spike dominated m.y and the
    limit is well below it, here  |m.y - w^2| <= w^2 / 4  and  L <= w / 4:  with R = |m.y - w^2| and y' <= R + L^2,
    D <= S u (w^2 + 2 R + (2 e_L / u + 2) L^2) <= S u w^2 (1 + 1/2 + 20/16) < 3 u w^2  even with e_L = 9u.  The last set of inputs is drawn for that premise (spikes
    ten times brighter), and every set must have such pixels.  Outside the premise 3 u w^2 does NOT hold (a limit near w puts (2 e_L + u) L^2 = 19 u w^2
    into D), which is why the header states D.
    The largest observed multiples are printed: x' 0.87, rho 0.58, c' 0.70, y' 0.95 of D and 0.32 of 3 u w^2 under the premise when this was written."""
    g = guides(w, h, 7 * w)
    worst = {"x'": 0.0, "rho": 0.0, "c'": 0.0, "y' / D": 0.0, "y' / (3u w^2), premise": 0.0}
    out_total = px_total = premise_total = 0
    for radius, scale, floor, seed, gain in ((1, 2.0, 0.0, 1, 1.0), (2, 1.0, 0.0, 2, 1.0), (3, 4.0, 0.05, 3, 1.0), (2, 2.0, 0.0, 4, 1.0), (2, 2.0, 0.0, 5, 10.0)):
        mean, m, _ = planted(w, h, seed, spikes=0.06, gain=gain)
        c32, m32, mask32 = run(hipmod, mean, g, m, N, scale, floor, radius, dem)
        mask32 = mask32 != 0
        r = firefly_ref.clamp64(mean, g["albedo"], g["kind"], m, N, scale, floor, radius, dem)
        close = np.abs(r["w"] - r["L"]) <= 4 * np.spacing(r["L"].astype(F)).astype(np.float64)
        assert np.array_equal(mask32[~close], r["mask"][~close]), f"radius {radius}: the decisions differ away from w == L"
        out_total, px_total = out_total + int(close.sum()), px_total + w * h
        on = mask32 & r["mask"] & ~close
        assert on.sum() > 20
        e_l = (9 if dem else 1) * U
        mx, my, wm, L = (m[..., 0].astype(np.float64), m[..., 1].astype(np.float64), r["w"], r["L"])
        tol_x = U * np.abs(mx - wm) + e_l * L + U * r["x1"]
        tol_rho = tol_x / mx + U * r["rho"]
        tol_c = np.abs(mean.astype(np.float64)) * tol_rho[..., None] + U * np.abs(r["c1"])
        tol_y = (1 + 32 * U) * (U * wm * wm + U * np.abs(my - wm * wm) + (2 * e_l + U) * L * L + U * r["y1"])
        premise = on & (np.abs(my - wm * wm) <= wm * wm / 4) & (L <= wm / 4)
        assert premise.sum() > (10 if gain > 1 else 0), f"radius {radius} scale {scale}: {int(premise.sum())} pixels under the premise"
        premise_total += int(premise.sum())
        rho32 = np.where(mx > 0, m32[..., 0].astype(np.float64) / mx, 0.0)              # (rho is not an output: x' / m.x in f64 from the f32 x' differs from it by u)
        for key, got, want, tol in (("x'", m32[..., 0], r["x1"], tol_x), ("rho", rho32, r["rho"], tol_rho), ("y' / D", m32[..., 1], r["y1"], tol_y)):
            ratio = (np.abs(got.astype(np.float64) - want)[on] / tol[on]).max()
            worst[key] = max(worst[key], float(ratio))
        worst["c'"] = max(worst["c'"], float((np.abs(c32.astype(np.float64) - r["c1"])[on] / np.maximum(tol_c[on], 1e-300)).max()))
        worst["y' / (3u w^2), premise"] = max(worst["y' / (3u w^2), premise"], float((np.abs(m32[..., 1].astype(np.float64) - r["y1"])[premise] / (3 * U * wm[premise] ** 2)).max()))
        assert np.allclose(m32[..., 3][on], L[on], rtol=2 * e_l, atol=0) and (m32[..., 2][on] == N).all()
    share = out_total / px_total
    print(f"{w}x{h} demodulated {dem}: {100 * share:.3f} % of the pixels left out (|w - L| <= 4 ulp); {premise_total} clamped pixels under the premise of 3u w^2; "
          "largest multiples of the bounds: " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert share <= 0.01
    assert all(v <= 1.0 for v in worst.values()), worst
