"""The variance-guided filter without a GPU: the host build of csrc/k_denoise.h dn_filter_pixel_var (hipmod.denoise_variance_host) against the numpy
restatement of tests/denoise_var_ref.py, bit for bit; its reduction to the plain filter; what the variance does to an edge; how the variance itself
propagates; and the shipped defaults against converged oracle images."""
import os

import numpy as np
import pytest

import denoise_ref
import denoise_var_ref
from conftest import ROOT, rel_l2

F = np.float32
SIZES = [(37, 23), (130, 67)]                         # (width, height); step 32 of the sixth pass exceeds both extents of the first


def guides_for(w, h, seed):
    """guide buffers with every kind in patches (so that taps do join), tilted normals, a few zero normals, albedos on both sides of the 0.01 floor"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    kind = ((xs // 7 + ys // 5 + (rng.random((h, w)) < 0.05)) % 3).astype(np.uint32)
    normal = rng.normal(size=(h, w, 3)).astype(F) * F(0.2) + np.array([0.0, 0.3, -1.0], F)
    normal = (normal / np.linalg.norm(normal, axis=-1, keepdims=True)).astype(F)
    normal[kind == 0] = 0.0
    normal[rng.random((h, w)) < 0.02] = 0.0
    depth = (3.0 + 0.01 * xs + 0.02 * ys + rng.random((h, w)) * 0.05).astype(F)
    depth[kind == 0] = 1e6
    position = (np.stack([xs * 0.01, ys * 0.01, np.zeros_like(xs, float)], -1) * depth[..., None]).astype(F)
    albedo = rng.choice(np.array([0.0, 0.004, 0.01, 0.2, 0.8, 1.0], F), (h, w, 3))
    albedo[kind != 1] = 1.0
    return {"albedo": albedo, "normal": normal, "position": position, "depth": depth, "kind": kind}


def image_and_moments(w, h, seed, hostile):
    """a noisy image with the moments record of its samples: per pixel n in {0, 1, 2, 3, 8} gamma-distributed samples added by mo_add, the mean of which is the
    image (0 for n = 0).  hostile: some colours NaN / inf / huge / negative, some records with non-finite or inconsistent sums."""
    rng = np.random.default_rng(seed)
    n = rng.choice(np.array([0, 1, 2, 3, 8]), (h, w), p=[0.05, 0.1, 0.25, 0.3, 0.3])
    sums, moments = np.zeros((h, w, 3), F), np.zeros((h, w, 4), F)
    scale = (0.1 + 2.0 * rng.random((h, w, 1))).astype(F)
    for k in range(8):
        live = (n > k)[..., None]
        s = np.where(live, rng.gamma(1.5, 0.4, (h, w, 3)).astype(F) * scale, F(0.0)).astype(F)
        m2 = denoise_var_ref.moments_add(moments.copy(), s)
        moments = np.where(live, m2, moments).astype(F)
        sums = (sums + s).astype(F)
    with np.errstate(all="ignore"):
        mean = np.where((n > 0)[..., None], sums / np.maximum(n, 1).astype(F)[..., None], F(0.0)).astype(F)
    if hostile:
        vals = np.array([np.nan, np.inf, -np.inf, 3e38, -1.0, 1e-42, 0.0], F)
        bad = rng.random((h, w)) < 0.08
        mean[bad] = vals[rng.integers(0, len(vals), (int(bad.sum()), 3))]
        recs = np.array([[np.inf, 1.0, 4.0, 1.0], [1.0, np.nan, 4.0, 1.0], [2.0, np.inf, 8.0, 1.0], [4.0, 1.0, 4.0, 1.0],      # the last: sum(Y^2) < sum(Y)^2 / n
                         [1e30, 1e30, 2.0, 1e30], [0.5, 0.3, np.inf, 0.5], [0.5, 0.3, np.nan, 0.5], [3.0, 9.0, 1.0, 3.0], [-np.inf, 2.0, 3.0, 0.0]], F)
        bad = rng.random((h, w)) < 0.08
        moments[bad] = recs[rng.integers(0, len(recs), int(bad.sum()))]
    return mean, moments


def assert_same_bits(got, want, what):
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), what
    differ = got[~ng].view(np.uint32) != want[~nw].view(np.uint32)
    assert not differ.any(), f"{what}: {np.count_nonzero(differ)} words differ"


def run_host(hipmod, img, g, moments, p, op=0):
    return hipmod.denoise_variance_host(img, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], moments, p, op)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("hostile", [False, True])
def test_host_hook_equals_the_numpy_restatement_bitwise(hipmod, oracle, w, h, hostile):
    """colour and variance; 1, 2 and 6 passes, both demodulation settings, several widths of the luminance term (0 and +inf among them)"""
    g = guides_for(w, h, w * 1000 + h)
    img, moments = image_and_moments(w, h, w + 7, hostile)
    v0 = denoise_var_ref.variance_of_mean(moments)
    assert np.isinf(v0).any() and (v0 == 0).sum() >= 0 and (np.isfinite(v0) & (v0 > 0)).sum() > w * h // 3        # known and unknown variances meet
    cases = [(it, dem, sv, 1.0) for it in (1, 2, 6) for dem in (0, 1) for sv in ((1.0, 4.0) if it != 2 else (0.25, 16.0))]
    cases += [(2, 1, float("inf"), 1.0), (2, 0, 0.0, 1.5), (6, 1, 2.0, 0.0), (0, 1, 1.0, 1.0)]
    for k, (it, dem, sv, sc) in enumerate(cases):
        p = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_variance=sv, sigma_color=sc, normal_power_log2=k % 3)
        op = k % 7
        got_rgb, got_var = run_host(hipmod, img, g, moments, p, op)
        want_rgb, want_var = denoise_var_ref.denoise_variance(img, g, moments, p, op, oracle)
        what = f"{w}x{h} hostile {hostile} iterations {it} demodulate {dem} sigma_variance {sv} sigma_color {sc} op {op}"
        assert_same_bits(got_rgb, want_rgb, what + ": colour")
        assert_same_bits(got_var, want_var, what + ": variance")
        assert not np.isnan(got_var).any() and (got_var[np.isfinite(got_var)] >= 0).all(), what       # a variance is >= 0 or unknown, never NaN
        assert np.array_equal(np.isinf(got_var), np.isinf(v0)) or hostile or dem, what                 # known iff the pixel's own record was (overflow apart)


@pytest.mark.parametrize("w,h", SIZES)
def test_without_the_term_it_is_the_plain_filter_bitwise(hipmod, w, h):
    """sigma_variance = 0, and sigma_variance > 0 over records that are all unmeasured: the RGB of rpt_debug_denoise_host with `base`"""
    g = guides_for(w, h, 11)
    img, moments = image_and_moments(w, h, 12, True)
    unmeasured = moments.copy()
    unmeasured[..., 2] = np.where(np.nan_to_num(unmeasured[..., 2], nan=0.0, posinf=0.0) >= 2, F(1.0), unmeasured[..., 2])
    unmeasured[np.isnan(unmeasured[..., 2]) | np.isinf(unmeasured[..., 2]), 2] = 0.0
    assert not (unmeasured[..., 2] >= 2).any()
    for it, dem, sc, op in [(1, 0, 1.0, 0), (2, 1, 1.0, 3), (6, 1, 0.7, 5), (3, 0, 0.0, 1), (0, 1, 1.0, 2)]:
        base = dict(iterations=it, demodulate=dem, sigma_color=sc)
        plain = hipmod.denoise_host(img, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], hipmod.denoise_params(**base), op)
        off, _ = run_host(hipmod, img, g, moments, hipmod.denoise_var_params(sigma_variance=0.0, **base), op)
        assert_same_bits(off, plain, f"sigma_variance 0, {base}")
        for sv in (1.0, float("inf")):
            blind, var = run_host(hipmod, img, g, unmeasured, hipmod.denoise_var_params(sigma_variance=sv, **base), op)
            assert_same_bits(blind, plain, f"unmeasured records, sigma_variance {sv}, {base}")
            assert np.isinf(var).all()
    # (the term does something where it is on: the comparison above is not vacuous)
    on, _ = run_host(hipmod, img, g, moments, hipmod.denoise_var_params(sigma_variance=1.0, iterations=2), 0)
    plain = hipmod.denoise_host(img, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], hipmod.denoise_params(iterations=2), 0)
    assert (on != plain).any(axis=-1).mean() > 0.3


def flat_scene(w, h):
    """one kind, one plane facing the camera, one normal: the normal weight is 1 and the plane distance 0 for every tap, bit for bit"""
    ys, xs = np.mgrid[0:h, 0:w]
    return {"albedo": np.ones((h, w, 3), F), "normal": np.broadcast_to(np.array([0.0, 0.0, -1.0], F), (h, w, 3)).copy(),
            "position": np.stack([xs * 0.01, ys * 0.01, np.full((h, w), 3.0)], -1).astype(F), "depth": np.full((h, w), 3.0, F), "kind": np.ones((h, w), np.uint32)}


def uniform_moments(w, h, v):
    """records of two samples whose variance of the mean is v: max(0, 2v - 0 * 0 / 2) / (2 * 1) = v exactly"""
    m = np.zeros((h, w, 4), F)
    m[..., 1], m[..., 2] = F(2.0) * F(v), 2.0
    return m


def test_the_variance_drives_the_edge_stop(hipmod):
    """A vertical luminance step of height 0.75 (0.25 | 1.0) on a flat wall, the colour term OFF: nothing but d_l can tell the two sides apart.
    Zero variance everywhere (a converged edge): the width is 1e-6, no tap crosses, and every pixel stays within 2^-22 relative of its input.
    Variance >= (step height)^2 (noise of the size of the step): the two columns next to the edge move strictly towards each other."""
    w, h, edge, step = 40, 24, 19, F(0.75)
    g = flat_scene(w, h)
    img = np.full((h, w, 3), F(0.25))
    img[:, edge:] = F(0.25) + step
    for it in (1, 3):
        p = hipmod.denoise_var_params(iterations=it, demodulate=0, sigma_color=0.0, sigma_variance=1.0)
        out, var = run_host(hipmod, img, g, uniform_moments(w, h, 0.0), p, 0)
        rel = np.abs(out.astype(np.float64) - img) / img
        print(f"{it} passes, zero variance: max relative change {rel.max():.3e} (bound {2.0 ** -22:.3e})")
        assert rel.max() <= 2.0 ** -22 and (var == 0).all()
        for v in (float(step) ** 2, 4.0):
            out, var = run_host(hipmod, img, g, uniform_moments(w, h, v), p, 0)
            left, right = out[:, edge - 1], out[:, edge]
            print(f"{it} passes, variance {v:g}: the columns at the edge go from 0.25 | 1.0 to {left[h // 2, 0]:.4f} | {right[h // 2, 0]:.4f}")
            assert (left > F(0.25)).all() and (right < F(1.0)).all() and (left < right).all()
            assert np.isfinite(var).all() and (var < F(v)).all()                              # (filtering shrinks the variance)
    # the plain filter with its colour term off blurs the converged edge: that is the difference
    plain = hipmod.denoise_host(img, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], hipmod.denoise_params(iterations=1, demodulate=0, sigma_color=0.0), 0)
    assert (plain[:, edge - 1] > F(0.25)).all()


def test_the_variance_propagates_as_the_squared_weights_say(hipmod):
    """constant colour, flat guides, uniform variance v, one pass: every weight is its kernel value k, sum(k) = 1, and an interior pixel returns
    v sum(k^2) = v (sum h^2)^2 = v (70/256)^2 = v 4900/65536.  k and k^2 are exact in f32 and so are the partial sums of k; what rounds is each product
    (k k) v and each of the 25 additions into the sum: 50 roundings, 50 x 2^-24 relative at the most (the terms are positive).  v = 0.5: nothing rounds."""
    w, h = 21, 13
    g = flat_scene(w, h)
    img = np.full((h, w, 3), F(0.6))
    for v, bound in ((0.5, 0.0), (0.37, 50 * 2.0 ** -24), (1e-9, 50 * 2.0 ** -24)):
        p = hipmod.denoise_var_params(iterations=1, demodulate=0, sigma_variance=2.0)
        _, var = run_host(hipmod, img, g, uniform_moments(w, h, v), p, 0)
        want = float(F(v)) * 4900.0 / 65536.0
        rel = np.abs(var[2:-2, 2:-2].astype(np.float64) - want) / want
        print(f"v {v:g}: interior variance {var[h // 2, w // 2]:.9g}, expected {want:.9g}, max relative deviation {rel.max():.3e} (bound {bound:.3e})")
        assert rel.max() <= bound
        assert (var[0] > var[h // 2, w // 2]).all()                                            # fewer taps at the border: less averaging


def test_parameter_checks(hipmod):
    g = flat_scene(8, 8)
    img, m = np.full((8, 8, 3), F(0.5)), uniform_moments(8, 8, 0.1)
    run_host(hipmod, img, g, m, hipmod.denoise_var_params(sigma_variance=float("inf"), iterations=6))
    for bad in (dict(sigma_variance=-1.0), dict(sigma_variance=float("nan")), dict(iterations=7), dict(sigma_color=-1.0)):
        with pytest.raises(hipmod.RptError) as e:
            run_host(hipmod, img, g, m, hipmod.denoise_var_params(**bad))
        assert e.value.code == -1, bad
    with pytest.raises(hipmod.RptError):
        run_host(hipmod, img, g, m, None, op=7)
    d = hipmod.denoise_var_params()
    assert d.sigma_variance >= 0 and 1 <= d.base.iterations <= 6


def test_the_shipped_defaults_are_no_worse_than_the_plain_filters(rpt, hipmod, world, oracle):
    """On the oracle images of the plain filter's quality test (DarkCornell, VeachMIS with NEE, PBRTest; 8 spp against 1024 spp, 128 x 128) and the moments
    of the 8-spp image's samples: the summed rel-L2 ratio at rpt_denoise_var_params_default is <= that of rpt_denoise's defaults — the plain default point is
    in the grid the shipped point is the minimum of (profiles/r14_denoise_variance_quality.txt).  Per scene the figures are printed, not asserted."""
    total_var = total_plain = 0.0
    for scene, nee in denoise_ref.QUALITY:
        noisy, conv, g, moments, sums = denoise_var_ref.quality_inputs(rpt, world, oracle, scene, nee)
        cfg = rpt.default_config(128, 128, nee=nee)
        direct, _, _ = oracle.trace_cpu(cfg, oracle.scene(world(scene)), rpt.blue_noise_seeds(128, 128), 8)
        assert_same_bits(sums, direct, f"{scene}: the eight single samples add up to the 8-spp accumulator")      # the inputs ARE those of denoise_ref.quality_images
        assert (moments[..., 2] == 8).all()
        plain = hipmod.denoise_host(noisy, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], None, 0)
        var, _ = run_host(hipmod, noisy, g, moments, None, 0)
        e_noisy, e_plain, e_var = rel_l2(noisy, conv), rel_l2(plain, conv), rel_l2(var, conv)
        print(f"{scene} nee {nee}: rel-L2 noisy {e_noisy:.4f}; ratio rpt_denoise defaults {e_plain / e_noisy:.3f}, rpt_denoise_variance defaults {e_var / e_noisy:.3f}")
        assert np.isfinite(var).all()
        total_plain += e_plain / e_noisy
        total_var += e_var / e_noisy
    print(f"summed ratio: rpt_denoise {total_plain:.4f}, rpt_denoise_variance {total_var:.4f}")
    assert total_var <= total_plain


def test_quality_record_is_kept():
    text = open(os.path.join(ROOT, "profiles", "r14_denoise_variance_quality.txt")).read()
    assert all(s in text for s in ("DarkCornell", "VeachMIS", "PBRTest", "sigma_variance")) and "grid" in text
