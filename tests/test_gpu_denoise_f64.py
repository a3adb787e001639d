"""The denoisers and the noise estimate ON THE DEVICE against the independent float64 statement of tests/denoise_f64.py: rpt_denoise, rpt_denoise_variance
(term on and off), rpt_denoise_temporal, rpt_read_noise and rpt_noise_count.  The device's own results on the device's own inputs — the accumulator, the
guides and the moments record are read back and taken as given by the float64 side.  Tolerances and bounds are those of tests/denoise_f64_cases.py, measured
on the CPU against the host hooks (which the device equals bit for bit by tests/test_gpu_denoise*.py); each test prints its own worst values.

Every case asserts: the flagged share is within the cap, more than 90 % of the pixels are compared, and everything is finite where float64 is.

Where the luminance term really works here: rpt_denoise_variance on DarkCornell and VeachMIS (sigma_variance 4), and rpt_denoise_temporal on VeachMIS alone.  On
the textured scene the filter runs at sigma_variance 32, where d_l is near 0, and its temporal call at +inf; DarkCornell's temporal calls run with the term off
(tests/denoise_f64_cases.py RENDERS says why: the cap on the flagged share decides the case, never the reverse).  The temporal records are not compared: the
device returns none."""
import numpy as np
import pytest

import denoise_f64 as d64
import denoise_f64_cases as cases
from denoise_f64_cases import FLAGGED_CAP, assert_temporal, assert_variance, masked_max, rel_diff
from moments_ref import SampleBank

pytestmark = pytest.mark.gpu

F = np.float32
SPP = 8


@pytest.fixture(scope="module")
def r(hipmod):
    """a Renderer of the module's own: it keeps moments on, which the session's renderer must not"""
    r = hipmod.Renderer(0)
    yield r
    r.close()


def look(r, rpt, cfg, spp=SPP):
    """a new accumulator epoch under `cfg`"""
    r.set_config(cfg)
    r.reset(rpt.blue_noise_seeds(cfg.width, cfg.height))
    if spp:
        r.render(spp)


def begin(r, rpt, wld, cfg, spp=SPP):
    r.upload_scene(wld)
    r.set_config(cfg)
    r.set_moments(False)
    r.set_moments(True)
    r.temporal_reset()
    look(r, rpt, cfg, spp)


def inputs(r):
    """the device's accumulator as a mean (every pixel by its own count while the counts differ), its guides and its moments record"""
    acc, n = r.read_accum()
    if r.counts_uniform():
        mean = (acc[..., :3] / F(n)).astype(F)
    else:
        with np.errstate(all="ignore"):
            mean = np.where(acc[..., 3:] == 0, F(0.0), acc[..., :3] / acc[..., 3:]).astype(F)
    return mean, r.guides(), r.read_moments()


def check_filters(r, hipmod, sigma_variance, what):
    """rpt_denoise, rpt_denoise_variance with the term off and on, against float64 on what the device holds now"""
    mean, g, moments = inputs(r)
    pixels = mean.shape[0] * mean.shape[1]
    p = hipmod.denoise_params(iterations=2, demodulate=1)
    got, want = r.denoise(params=p, tonemap_op=3), d64.filter(mean, g, p, 3)
    d = float(rel_diff(got, want).max())
    print(f"{what}: rpt_denoise, largest relative difference {d:.3e} (tolerance {cases.PLAIN_TOL:.3e})")
    assert np.isfinite(got[np.isfinite(want)]).all() and d <= cases.PLAIN_TOL, what
    for it, dem, sv, op in [(2, 1, 0.0, 0), (2, 1, sigma_variance, 5), (3, 0, sigma_variance, 0)]:
        p = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_variance=sv)
        got, got_v = r.denoise_variance(params=p, tonemap_op=op)
        watch = cases.VarianceBound(moments)
        want, want_v, flagged = d64.filter_variance(mean, g, moments, p, op, watch=watch)
        case = f"{what}: rpt_denoise_variance iterations {it} demodulate {dem} sigma_variance {sv}"
        assert flagged.mean() <= FLAGGED_CAP and (~flagged).sum() > 0.9 * pixels, f"{case}: flagged {flagged.mean():.4f}"
        assert np.isfinite(got[np.isfinite(want) & ~flagged[..., None]]).all(), case
        d = masked_max(rel_diff(got, want), flagged)
        print(f"{case}: flagged {flagged.mean():.5f}, largest relative difference {d:.3e} (tolerance {cases.VARIANCE_TOL:.3e})")
        assert d <= cases.VARIANCE_TOL, case
        assert_variance(got_v, want_v, watch.of(want_v), flagged, case)


def temporal_step(r, hipmod, cfg, previous, p, op, what):
    """rpt_denoise_temporal against float64 on the device's inputs: colour, T, the reuse decisions and the count end to end; the variance end to end without
    passes, and with passes against float64 passes run from the blend itself (cases.passes_from_the_blend) — the host hook's records, which are the device's
    own history bit for bit (tests/test_gpu_denoise_temporal.py).  -> the history for the next view, from the same records"""
    mean, g, moments = inputs(r)
    rgb, var, hist, rep = r.denoise_temporal(params=p, tonemap_op=op, with_report=True)
    watch = cases.VarianceBound(moments)
    want = d64.temporal(mean, g, moments, cfg, previous, p, op, watch=watch)
    want["bound"] = watch.of(want["variance"])
    got = {"rgb": rgb, "variance": var, "history": hist, "pixels_with_history": rep["pixels_with_history"]}
    host = hipmod.denoise_temporal_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], moments, cfg, previous, p, op)
    d = assert_temporal(got, want, moments, p.filter.base.iterations, what, after=cases.passes_from_the_blend(host["records"], hist, moments, g, p, op))
    print(f"{what}: flagged {((want['margin'] < cases.DELTA) | want['flagged']).mean():.5f}, reused {want['pixels_with_history']} (device {rep['pixels_with_history']}), "
          f"colour {d['colour']:.3e} (tolerance {cases.TEMPORAL_TOL:.3e}), T {d['T']:.3e} (tolerance {cases.TEMPORAL_T_TOL:.3e})")
    return {"camera": cfg.copy(), "normal": g["normal"], "position": g["position"], "kind": g["kind"], "records": host["records"]}, want


@pytest.mark.parametrize("scene,nee,w,h,sigma_variance,sigma_temporal", cases.RENDERS)
def test_the_filters_and_one_reprojection_on_the_devices_own_inputs(r, rpt, hipmod, world, scene, nee, w, h, sigma_variance, sigma_temporal):
    """130 x 67 and 128 x 96: partial 64-pixel row segments, a height that is no multiple of 4; 70 x 9 and 1 x 1: partial 64 x 4 workgroups.  (The luminance
    term of the temporal call is effectively on for VeachMIS only: see the module's docstring.)"""
    cam_a, cam_b = cases.render_views(rpt, scene, nee, w, h)
    begin(r, rpt, cases.render_world(world, scene), cam_a)
    what = f"{scene} nee {nee} {w}x{h}"
    check_filters(r, hipmod, sigma_variance, what)
    p = hipmod.temporal_params(iterations=2, demodulate=1, sigma_variance=sigma_temporal, max_history=32.0, normal_min=0.9, plane_max=2.0)
    prev, first = temporal_step(r, hipmod, cam_a, None, p, 0, what + " A")
    assert first["pixels_with_history"] == 0
    look(r, rpt, cam_b)
    _, moved = temporal_step(r, hipmod, cam_b, prev, p, 3, what + " A->B")
    assert moved["pixels_with_history"] > 0 or w == 1


@pytest.mark.parametrize("scene,nee,w,h,sigma_variance,sigma_temporal", cases.RENDERS[:2])
def test_temporal_reuse_along_a_path(r, rpt, hipmod, world, scene, nee, w, h, sigma_variance, sigma_temporal):
    """A -> B -> B (a second call in B's epoch, after more samples: the same previous history) -> A"""
    cam_a, cam_b = cases.render_views(rpt, scene, nee, w, h)
    begin(r, rpt, cases.render_world(world, scene), cam_a)
    what = f"{scene} nee {nee}"
    p = hipmod.temporal_params(iterations=1, demodulate=0, sigma_variance=sigma_temporal, max_history=16.0, normal_min=0.8, plane_max=float("inf"))
    prev_a, _ = temporal_step(r, hipmod, cam_a, None, p, 1, what + " A")
    look(r, rpt, cam_b)
    _, b = temporal_step(r, hipmod, cam_b, prev_a, p, 2, what + " A->B")
    r.render(SPP)
    prev_b, b2 = temporal_step(r, hipmod, cam_b, prev_a, p, 4, what + " A->B->B")
    assert b2["pixels_with_history"] == b["pixels_with_history"] > 0 and b2["history"].max() <= 16 + 2 * SPP
    look(r, rpt, cam_a)
    _, back = temporal_step(r, hipmod, cam_a, prev_b, p, 6, what + " A->B->A")
    assert 0 < back["pixels_with_history"] < w * h


@pytest.mark.parametrize("scene,nee,w,h,sigma_variance,sigma_temporal", cases.RENDERS[:2])
def test_per_pixel_counts(r, rpt, hipmod, world, scene, nee, w, h, sigma_variance, sigma_temporal):
    """one rpt_render_pixels pass over half the image (a checkerboard) before denoising: every pixel's mean by its own count, its variance from its own record"""
    cam_a, cam_b = cases.render_views(rpt, scene, nee, w, h)
    begin(r, rpt, cases.render_world(world, scene), cam_a)
    p = hipmod.temporal_params(iterations=2, demodulate=1, sigma_variance=sigma_temporal, max_history=32.0, normal_min=0.9, plane_max=2.0)
    prev, _ = temporal_step(r, hipmod, cam_a, None, p, 0, f"{scene} A")
    look(r, rpt, cam_b)
    yy, xx = np.mgrid[0:h, 0:w]
    r.render_pixels((yy + xx) % 2 == 0, 5)
    assert not r.counts_uniform() and set(np.unique(r.read_moments()[..., 2])) == {8.0, 13.0}
    check_filters(r, hipmod, sigma_variance, f"{scene} nee {nee} checkerboard")
    temporal_step(r, hipmod, cam_b, prev, p, 3, f"{scene} nee {nee} checkerboard A->B")


@pytest.mark.parametrize("scene,nee,w,h,sigma_variance,sigma_temporal", cases.RENDERS[:2])
def test_the_noise_estimate_against_the_samples_in_float64(r, rpt, hipmod, oracle, world, scene, nee, w, h, sigma_variance, sigma_temporal):
    """rpt_read_noise and rpt_noise_count after 16 samples with moments on, against the float64 figures from the oracle's per-sample radiances: the bound of
    tests/test_denoise_f64.py's moments test; a pixel counts as above the threshold unless its float64 value is within the bound of it, and such pixels are
    at most the cap's share of the image"""
    n = 16
    cfg, _ = cases.render_views(rpt, scene, nee, w, h)
    begin(r, rpt, world(scene), cfg, n)
    bank = SampleBank(oracle, cfg, world(scene), rpt.blue_noise_seeds(w, h))
    bank.need(n)
    m64 = d64.moments_of_samples(np.stack(bank.radiance[:n]))
    v64, rel64 = d64.variance_of_mean(m64), d64.noise_rel(m64)
    bound = cases.noise_bound(m64, v64, rel64, cases.variance_bound(m64, v64, extra=n), extra=n)
    rel = r.read_noise()
    err = np.abs(d64.widen(rel) - rel64)
    print(f"{scene} nee {nee}: rpt_read_noise, largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert np.isfinite(rel).all() and (err <= bound).all()
    for threshold in cases.NOISE_THRESHOLDS[scene]:
        k = r.noise_count(threshold)
        surely, doubtful = int((rel64 > threshold + bound).sum()), int((np.abs(rel64 - threshold) <= bound).sum())
        print(f"{scene} nee {nee} threshold {threshold}: above {k['above']}, float64 {surely} and {doubtful} within the bound of the threshold")
        assert k["pixels"] == k["measured"] == w * h and doubtful <= FLAGGED_CAP * w * h
        assert surely <= k["above"] <= surely + doubtful
        assert 0 < surely < w * h
