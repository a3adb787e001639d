"""Temporal reuse without a GPU: the host build of csrc/k_temporal.h (hipmod.denoise_temporal_host) against the numpy restatement of tests/temporal_ref.py, bit for
bit — colour, variance, the blended count T and the new history records; its reduction to rpt_denoise_variance without a history; the identity path and the
blend's closed form; what rejects a history tap; the cap; the unknown variance; the f32 projection against float64; the refusals.

The views are of a small analytic room (a wall, a floor, an emitter on the wall, open sky at the sides), so that the previous view's guides and the current
ones describe the same surfaces and taps do join; the colours, moments and history records are random."""
import os

import numpy as np
import pytest

import denoise_ref
import temporal_ref
from conftest import ROOT
from test_denoise_variance import assert_same_bits, image_and_moments

F = np.float32
SIZES = [(37, 23), (130, 67)]
MOVED = dict(cam_position=(0.4, 0.1, 0.2, 0.0), cam_rotation=(-0.03, 0.08, 0.0, 0.0))       # sideways, up, forward; pitched and yawed


def camera(rpt, w, h, **changes):
    return rpt.default_config(w, h, **({"cam_position": (0.0, 0.0, 0.0, 0.0), "cam_rotation": (0.0, 0.0, 0.0, 0.0)} | changes))


def room(cfg, oracle, seed=0, zero_normals=False):
    """the guides of the room from `cfg`: wall z = 6 (|x| <= 5, y <= 4, beyond it sky) with an emitter |x| < 1, |y| < 0.5, floor y = -1.5 in front of it"""
    w, h = cfg.width, cfg.height
    ro, rd = denoise_ref.camera_rays(cfg, oracle)
    with np.errstate(all="ignore"):
        t_wall = np.where(rd[:, 2] > 0, (F(6.0) - ro[:, 2]) / rd[:, 2], F(np.inf)).astype(F)
        t_floor = np.where(rd[:, 1] < 0, (F(-1.5) - ro[:, 1]) / rd[:, 1], F(np.inf)).astype(F)
        floor = t_floor < t_wall
        t = np.where(floor, t_floor, t_wall).astype(F)
        p = (ro + rd * t[:, None]).astype(F)
    miss = ~np.isfinite(t) | (~floor & ((np.abs(p[:, 0]) > 5) | (p[:, 1] > 4)))
    t = np.where(miss, F(1e6), t).astype(F)
    p = (ro + rd * t[:, None]).astype(F)
    kind = np.where(miss, 0, np.where(~floor & (np.abs(p[:, 0]) < 1) & (np.abs(p[:, 1]) < 0.5), 2, 1)).astype(np.uint32)
    normal = np.where(floor[:, None], np.array([0, 1, 0], F), np.array([0, 0, -1], F)).astype(F)
    normal[miss] = 0
    rng = np.random.default_rng(seed)
    if zero_normals:
        normal[rng.random(w * h) < 0.02] = 0
    albedo = rng.choice(np.array([0.004, 0.2, 0.8, 1.0], F), (w * h, 3))
    albedo[kind != 1] = 1
    return {"albedo": albedo.reshape(h, w, 3), "normal": normal.reshape(h, w, 3), "position": p.reshape(h, w, 3), "depth": t.reshape(h, w), "kind": kind.reshape(h, w)}


def records(w, h, seed, hostile):
    """history records: N in {0 (a hole), 1, 3.5, 12, 40}, colours and per-sample moments of the size of the images'"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((h, w, 6), F)
    rec[..., :3] = rng.gamma(1.5, 0.4, (h, w, 3))
    rec[..., 3] = rng.choice(np.array([0, 1, 3.5, 12, 40], F), (h, w), p=[0.1, 0.2, 0.2, 0.3, 0.2])
    rec[..., 4] = rng.gamma(1.5, 0.4, (h, w))
    rec[..., 5] = rec[..., 4] ** 2 * (1 + rng.random((h, w)))
    if hostile:
        vals = np.array([np.nan, np.inf, -np.inf, 3e38, -1.0, 0.0], F)
        bad = rng.random((h, w)) < 0.1
        rec[bad] = vals[rng.integers(0, len(vals), (int(bad.sum()), 6))]
    return rec


def previous_of(cfg, g, rec):
    return {"camera": cfg, "normal": g["normal"], "position": g["position"], "kind": g["kind"], "records": rec}


def run(hipmod, img, g, moments, cam, prev, p, op=0):
    return hipmod.denoise_temporal_host(img, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], moments, cam, prev, p, op)


def assert_same(got, want, what):
    for k in ("rgb", "variance", "history", "records"):
        assert_same_bits(got[k], want[k], f"{what}: {k}")
    assert got["pixels_with_history"] == want["pixels_with_history"], what


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("hostile", [False, True])
def test_host_hook_equals_the_numpy_restatement_bitwise(rpt, hipmod, oracle, w, h, hostile):
    """view A -> a moved view B, A -> A (the identity path), and an all-miss pair of views; resolve only, 1 and 2 passes, both demodulation settings"""
    cam_a, cam_b = camera(rpt, w, h), camera(rpt, w, h, **MOVED)
    up = dict(cam_rotation=(-1.2, 0.0, 0.0, 0.0))                                                  # pitched towards the sky: every pixel a miss
    sky_a, sky_b = camera(rpt, w, h, **up), camera(rpt, w, h, cam_position=(0.3, 0.0, 0.0, 0.0), cam_rotation=(-1.2, 0.05, 0.0, 0.0))
    views = [("A->B", cam_a, cam_b), ("A->A", cam_a, cam_a), ("sky", sky_a, sky_b)]
    for name, c0, c1 in views:
        g0, g1 = room(c0, oracle, 1, hostile), room(c1, oracle, 2, hostile)
        assert (name == "sky") == (g1["kind"] == 0).all()
        img, moments = image_and_moments(w, h, w + 3, hostile)
        prev = previous_of(c0, g0, records(w, h, h + 5, hostile))
        cases = [(0, 1, 0.0), (1, 0, 4.0), (2, 1, 4.0)] if name == "A->B" else [(1, 1, 4.0)]
        for k, (it, dem, sv) in enumerate(cases):
            p = hipmod.temporal_params(iterations=it, demodulate=dem, sigma_variance=sv, max_history=[32.0, 8.0, float("inf")][k], normal_min=0.9, plane_max=[2.0, 0.5, float("inf")][k])
            got = run(hipmod, img, g1, moments, c1, prev, p, k)
            want = temporal_ref.denoise_temporal(img, g1, moments, c1, prev, p, k, oracle)
            what = f"{w}x{h} {name} hostile {hostile} iterations {it} demodulate {dem}"
            assert_same(got, want, what)
            n_cur = moments[..., 2]
            assert got["pixels_with_history"] == np.count_nonzero(got["history"] > n_cur) or hostile, what
            assert 0 < got["pixels_with_history"] < w * h, what                                   # pixels with history and without are both present


@pytest.mark.parametrize("w,h", SIZES)
def test_an_empty_history_is_the_variance_filter_bitwise(rpt, hipmod, oracle, w, h):
    """no previous view; a previous view whose records are all holes; max_history = 0: colour and variance of rpt_debug_denoise_variance_host, T = n_cur"""
    cam_a, cam_b = camera(rpt, w, h), camera(rpt, w, h, **MOVED)
    g0, g1 = room(cam_a, oracle, 1), room(cam_b, oracle, 2)
    img, moments = image_and_moments(w, h, 9, True)
    holes = records(w, h, 4, False)
    holes[..., 3] = 0
    for it, dem, sv, op in [(0, 1, 0.0, 2), (1, 0, 4.0, 0), (3, 1, 2.0, 3)]:
        vp = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_variance=sv)
        want_rgb, want_var = hipmod.denoise_variance_host(img, g1["albedo"], g1["normal"], g1["position"], g1["depth"], g1["kind"], moments, vp, op)
        for prev, cap in [(None, 32.0), (previous_of(cam_a, g0, holes), 32.0), (previous_of(cam_a, g0, records(w, h, 4, False)), 0.0)]:
            p = hipmod.temporal_params(iterations=it, demodulate=dem, sigma_variance=sv, max_history=cap)
            got = run(hipmod, img, g1, moments, cam_b, prev, p, op)
            assert_same_bits(got["rgb"], want_rgb, "colour")
            assert_same_bits(got["variance"], want_var, "variance")
            assert_same_bits(got["history"], moments[..., 2], "T")
            assert got["pixels_with_history"] == 0


def flat_inputs(w, h, n_cur, y_cur):
    """a grey image of luminance y_cur whose records hold n_cur equal samples"""
    img = np.full((h, w, 3), F(y_cur))
    m = np.zeros((h, w, 4), F)
    y = temporal_ref.denoise_var_ref.luminance(img).astype(F)
    for _ in range(n_cur):
        m[..., 0] = m[..., 0] + y
        m[..., 1] = m[..., 1] + y * y
        m[..., 2] += 1
    return img, m


def flat_records(w, h, n, e, mu1, mu2):
    rec = np.zeros((h, w, 6), F)
    rec[..., :3], rec[..., 3], rec[..., 4], rec[..., 5] = e, n, mu1, mu2
    return rec


def test_identical_cameras_take_the_identity_path_and_the_blend_is_the_closed_form(rpt, hipmod, oracle):
    """the same camera twice: every pixel's one tap is itself with weight 1, so e_r, mu_r and N_r are the records' own and
    e = (N e_h + n e_cur) / T, mu = (N mu_r + m) / T, v = max(0, mu2 - mu1^2) / (T - 1), T = N + n, evaluated here in f32 in that order"""
    w, h = 37, 23
    cam = camera(rpt, w, h)
    g = room(cam, oracle)
    img, m = flat_inputs(w, h, 2, 0.5)
    N, e_h, mu1_h, mu2_h = F(4.0), F(0.2), F(0.25), F(0.1)
    p = hipmod.temporal_params(iterations=0, max_history=32.0)
    got = run(hipmod, img, g, m, cam, previous_of(cam, g, flat_records(w, h, N, e_h, mu1_h, mu2_h)), p)
    T = F(N + F(2.0))
    e = F(F(F(N * e_h) + F(F(2.0) * F(0.5))) / T)
    mu1 = F(F(F(N * mu1_h) + m[0, 0, 0]) / T)
    mu2 = F(F(F(N * mu2_h) + m[0, 0, 1]) / T)
    v = F(max(F(mu2 - F(mu1 * mu1)), F(0.0)) / F(T - F(1.0)))
    assert got["pixels_with_history"] == w * h and (got["history"] == T).all()
    assert (got["records"] == np.array([e, e, e, T, mu1, mu2], F)).all()
    assert (got["rgb"] == e).all() and (got["variance"] == v).all() and v > 0
    # a yaw of 1e-4 more is another camera: the bilinear path, four taps of the same flat records — the same image up to the rounding of the weights' sum
    turned = camera(rpt, w, h, cam_rotation=(0.0, 1e-4, 0.0, 0.0))
    other = run(hipmod, img, g, m, cam, previous_of(turned, g, flat_records(w, h, N, e_h, mu1_h, mu2_h)), p)
    assert other["pixels_with_history"] == w * h and not np.array_equal(other["records"], got["records"])
    assert np.abs(other["rgb"].astype(np.float64) - float(e)).max() <= 4 * 2.0 ** -24


def test_each_rule_rejects(rpt, hipmod, oracle):
    """behind the previous camera; another kind; the normal test; the plane test — each alone turns reuse off for the pixels it concerns, and only for them"""
    w, h = 37, 23
    cam = camera(rpt, w, h)
    g = room(cam, oracle)
    img, m = flat_inputs(w, h, 2, 0.5)
    rec = flat_records(w, h, 4.0, 0.2, 0.25, 0.1)
    p = hipmod.temporal_params(iterations=0, max_history=32.0, normal_min=0.9, plane_max=2.0)
    full = run(hipmod, img, g, m, cam, previous_of(cam, g, rec), p)
    assert full["pixels_with_history"] == w * h
    # a previous camera that looked the other way: every point of this view is behind it
    back = camera(rpt, w, h, cam_rotation=(0.0, float(np.pi), 0.0, 0.0))
    assert run(hipmod, img, g, m, cam, previous_of(back, g, rec), p)["pixels_with_history"] == 0
    hits = g["kind"] != 0
    # the previous view saw another kind in one column
    other = {k: v.copy() for k, v in g.items()}
    other["kind"][:, 10] = (g["kind"][:, 10] + 1) % 3
    got = run(hipmod, img, g, m, cam, previous_of(cam, other, rec), p)
    assert np.array_equal(got["history"] > 2, np.arange(w)[None, :].repeat(h, 0) != 10)
    # ... a normal tilted by more than acos(0.9) there (misses have no normal test)
    other = {k: v.copy() for k, v in g.items()}
    c, s = F(np.cos(0.5)), F(np.sin(0.5))                                                        # about the x axis: n . n' = cos(0.5) = 0.878 for wall and floor
    n = g["normal"][:, 10]
    other["normal"][:, 10] = np.stack([n[:, 0], c * n[:, 1] - s * n[:, 2], s * n[:, 1] + c * n[:, 2]], -1)
    got = run(hipmod, img, g, m, cam, previous_of(cam, other, rec), p)
    assert np.array_equal(got["history"][:, 10] > 2, ~hits[:, 10]) and (np.delete(got["history"], 10, 1) > 2).all()
    assert (run(hipmod, img, g, m, cam, previous_of(cam, other, rec), hipmod.temporal_params(iterations=0, normal_min=0.8))["history"] > 2).all()
    # ... a surface three footprints off the centre's tangent plane there (2 / w * t per footprint), under plane_max = 2; four allow it
    other = {k: v.copy() for k, v in g.items()}
    other["position"][:, 10] = g["position"][:, 10] + g["normal"][:, 10] * (F(3.0) * F(2.0 / w) * g["depth"][:, 10])[:, None]
    got = run(hipmod, img, g, m, cam, previous_of(cam, other, rec), p)
    assert np.array_equal(got["history"][:, 10] > 2, ~hits[:, 10]) and hits[:, 10].any()
    assert (run(hipmod, img, g, m, cam, previous_of(cam, other, rec), hipmod.temporal_params(iterations=0, plane_max=4.0))["history"] > 2).all()


def test_the_cap_and_the_unknown_variance(rpt, hipmod, oracle):
    w, h = 37, 23
    cam = camera(rpt, w, h)
    g = room(cam, oracle)
    img, m = flat_inputs(w, h, 2, 0.5)
    prev = previous_of(cam, g, flat_records(w, h, 40.0, 0.2, 0.25, 0.1))
    for cap, want in [(8.0, 10.0), (40.0, 42.0), (float("inf"), 42.0), (0.5, 2.5)]:
        got = run(hipmod, img, g, m, cam, prev, hipmod.temporal_params(iterations=0, max_history=cap))
        assert (got["history"] == F(want)).all() and (got["records"][..., 3] == F(want)).all(), cap
    # T < 2: one current sample and half a sample of history give T = 1.5 and no variance; T = 2 gives one
    img1, m1 = flat_inputs(w, h, 1, 0.5)
    got = run(hipmod, img1, g, m1, cam, prev, hipmod.temporal_params(iterations=2, max_history=0.5))
    assert (got["history"] == F(1.5)).all() and np.isinf(got["variance"]).all() and got["pixels_with_history"] == w * h
    got = run(hipmod, img1, g, m1, cam, prev, hipmod.temporal_params(iterations=0, max_history=1.0))
    assert (got["history"] == F(2.0)).all() and np.isfinite(got["variance"]).all()
    # ... which the pixel's own record could not have given: rpt_denoise_variance has no variance after one sample
    alone = hipmod.denoise_variance_host(img1, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], m1, hipmod.denoise_var_params(iterations=0), 0)
    assert np.isinf(alone[1]).all()
    # a current mean that is not finite passes through and leaves no history
    bad = img.copy()
    bad[3, 4, 1] = np.nan
    got = run(hipmod, bad, g, m, cam, prev, hipmod.temporal_params(iterations=0))
    assert np.isnan(got["rgb"][3, 4, 1]) and got["records"][3, 4, 3] == 0 and got["history"][3, 4] == 2 and got["pixels_with_history"] == w * h - 1


def test_the_f32_projection_against_float64(rpt, oracle):
    """tp_project in f32 (the rotation matrix from the library's f32 sine and cosine) against the same projection in float64 from the angles, over the
    pixels of views A and the sky pair of 130 x 67 that land inside the previous image: the largest difference measured is 1.84e-5 pixels in x or y
    (a screen coordinate of up to 130 carries 2^-24 relative error per f32 operation, 7.7e-6 pixels each, over a dozen operations); asserted: 4 x that,
    7.4e-5 pixels."""
    w, h = 130, 67
    worst = 0.0
    for c0, c1 in [(camera(rpt, w, h), camera(rpt, w, h, **MOVED)), (camera(rpt, w, h, cam_rotation=(-1.2, 0.0, 0.0, 0.0)), camera(rpt, w, h, cam_position=(0.3, 0.0, 0.0, 0.0), cam_rotation=(-1.2, 0.05, 0.0, 0.0)))]:
        g = room(c1, oracle)
        fx, fy, ok = temporal_ref.project(g["position"], g["kind"], temporal_ref.camera_position(c1), temporal_ref.camera_position(c0), temporal_ref.camera_matrix(c0, oracle), w, h)
        fx64, fy64, front = temporal_ref.project64(g["position"], g["kind"], c1, c0)
        assert ok.sum() > w * h // 3 and front[ok].all()
        worst = max(worst, np.abs(fx[ok] - fx64[ok]).max(), np.abs(fy[ok] - fy64[ok]).max())
    print(f"largest difference between the f32 and the float64 projection: {worst:.3e} pixels (measured 1.84e-5, bound 7.4e-5)")
    assert worst <= 7.4e-5


def test_parameter_checks(rpt, hipmod, oracle):
    w, h = 8, 8
    cam = camera(rpt, w, h)
    g = room(cam, oracle)
    img, m = flat_inputs(w, h, 2, 0.5)
    prev = previous_of(cam, g, flat_records(w, h, 4.0, 0.2, 0.25, 0.1))
    run(hipmod, img, g, m, cam, prev, hipmod.temporal_params(max_history=float("inf"), plane_max=float("inf"), normal_min=-1.0))
    run(hipmod, img, g, m, cam, prev, None)
    for bad in (dict(max_history=-1.0), dict(max_history=float("nan")), dict(plane_max=-0.5), dict(plane_max=float("nan")), dict(normal_min=float("nan")),
                dict(normal_min=1.5), dict(normal_min=-1.5), dict(sigma_variance=-1.0), dict(iterations=7)):
        with pytest.raises(hipmod.RptError) as e:
            run(hipmod, img, g, m, cam, prev, hipmod.temporal_params(**bad))
        assert e.value.code == -1, bad
    with pytest.raises(hipmod.RptError):
        run(hipmod, img, g, m, cam, prev, None, op=7)
    with pytest.raises(hipmod.RptError):
        run(hipmod, img, g, m, camera(rpt, w + 1, h), prev, None)
    d = hipmod.temporal_params()
    assert d.max_history > 0 and -1 <= d.normal_min <= 1 and d.plane_max > 0 and 1 <= d.filter.base.iterations <= 6


def test_the_shipped_defaults_are_the_minimum_of_the_kept_grid(hipmod):
    """profiles/r15_temporal_quality.txt: the first row of the sorted grid is rpt_temporal_params_default, and temporal reuse beats both single-frame filters there"""
    text = open(os.path.join(ROOT, "profiles", "r15_temporal_quality.txt")).read()
    assert all(s in text for s in ("DarkCornell", "VeachMIS", "PBRTest", "max_history")) and "not a grid point" not in text
    lines = text.splitlines()
    first = lines[[k for k, l in enumerate(lines) if l.startswith("grid (sorted")][0] + 1].split("|")[0].split()
    d = hipmod.temporal_params()
    assert [float(v) for v in first] == [d.max_history, d.normal_min, d.plane_max, d.filter.sigma_variance, float(d.filter.base.iterations)]
    total = lambda name: float([l for l in lines if l.startswith(name)][0].rsplit("|", 1)[1])
    assert total("rpt_denoise_temporal") < min(total("rpt_denoise,"), total("rpt_denoise_variance,"))
