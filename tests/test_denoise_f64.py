"""The denoisers and the noise estimate without a GPU, against an INDEPENDENT float64 statement (tests/denoise_f64.py, written from DESIGN.md and the header
comments): the host builds of csrc/k_denoise.h, k_temporal.h and k_moments.h — which the device equals bit for bit (tests/test_gpu_denoise*.py,
test_gpu_moments.py) — within tolerances measured once on the CPU, and within derived bounds for the variance (tests/denoise_f64_cases.py says how).
Beside it two checks that are independent even of that statement: the reprojection against the geometry of the views, and the moments against the
oracle's per-sample radiances."""
import numpy as np
import pytest

import denoise_f64 as d64
import denoise_f64_cases as cases
import denoise_ref
from denoise_f64_cases import DELTA, FLAGGED_CAP, SIZES, assert_temporal, assert_variance, masked_max, rel_diff
from moments_ref import SampleBank

F = np.float32


def planes(g):
    return g["albedo"], g["normal"], g["position"], g["depth"], g["kind"]


def host_variance(hipmod, rec):
    """mo_variance_of_mean of the records (..., 4) through rpt_debug_denoise_variance_host: without passes its variance plane is the pre-pass's"""
    flat = np.ascontiguousarray(rec, F).reshape(-1, 4)
    w = 1024
    rows = -(-len(flat) // w)
    m = np.zeros((rows * w, 4), F)
    m[:len(flat)] = flat
    z = np.zeros((rows, w, 3), F)
    v = hipmod.denoise_variance_host(z, z + 1, z, z, z[..., 0] + 1, np.ones((rows, w), np.uint32), m.reshape(rows, w, 4), hipmod.denoise_var_params(iterations=0), 0)[1]
    return v.reshape(-1)[:len(flat)].reshape(np.shape(rec)[:-1])


# ---- the filters ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", SIZES)
def test_the_plain_filter_against_float64(hipmod, w, h):
    img, g, _ = cases.filter_inputs(w, h)
    worst = 0.0
    for it, dem, sc, _, npl, op in cases.FILTER_CASES:
        p = hipmod.denoise_params(iterations=it, demodulate=dem, sigma_color=sc, normal_power_log2=npl)
        got, want = hipmod.denoise_host(img, *planes(g), p, op), d64.filter(img, g, p, op)
        d = float(rel_diff(got, want).max())
        worst = max(worst, d)
        assert np.isfinite(got[np.isfinite(want)]).all()
        assert d <= cases.PLAIN_TOL, f"{w}x{h} iterations {it} demodulate {dem} sigma_color {sc} normal_power_log2 {npl} op {op}: {d:.3e}"
    print(f"{w}x{h}: largest relative difference {worst:.3e} (measured {cases.PLAIN_REL_MAX:.3e}, tolerance {cases.PLAIN_TOL:.3e})")


@pytest.mark.parametrize("w,h", SIZES)
def test_the_variance_filter_against_float64(hipmod, w, h):
    img, g, moments = cases.filter_inputs(w, h)
    worst = 0.0
    for it, dem, sc, sv, npl, op in cases.FILTER_CASES:
        what = f"{w}x{h} iterations {it} demodulate {dem} sigma_color {sc} sigma_variance {sv} normal_power_log2 {npl} op {op}"
        p = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_color=sc, normal_power_log2=npl, sigma_variance=sv)
        got, got_v = hipmod.denoise_variance_host(img, *planes(g), moments, p, op)
        watch = cases.VarianceBound(moments)
        want, want_v, flagged = d64.filter_variance(img, g, moments, p, op, watch=watch)
        assert flagged.mean() <= FLAGGED_CAP and (~flagged).mean() > 0.9, what
        assert np.isfinite(got[np.isfinite(want)]).all(), what
        d = masked_max(rel_diff(got, want), flagged)
        worst = max(worst, d)
        assert d <= cases.VARIANCE_TOL, f"{what}: {d:.3e}"
        assert_variance(got_v, want_v, watch.of(want_v), flagged, what)
        if sv == 0.0:                                                                       # the plain filter is the variance filter without the term
            assert np.array_equal(want, d64.filter(img, g, p.base, op), equal_nan=True)
    print(f"{w}x{h}: largest relative difference {worst:.3e} (measured {cases.VARIANCE_REL_MAX:.3e}, tolerance {cases.VARIANCE_TOL:.3e})")


def test_the_variance_of_the_mean_and_noise_rel_within_their_derived_bounds(hipmod):
    """from given f32 records: the synthetic images' and 10^5 random ones with 2 to 200 samples whose luminances nearly agree (where the one-pass formula
    cancels: relatively the variance is then off by anything, absolutely it stays within c 2^-24 sum(Y^2) / (n (n - 1)))"""
    rng = np.random.default_rng(5)
    n = rng.integers(2, 200, 100000).astype(np.float64)
    y = rng.gamma(1.5, 0.4, len(n))
    spread = y * 10.0 ** rng.uniform(-6, 0, len(n))
    rec = np.stack([n * y, n * (y * y + spread * spread), n, y], -1).astype(F)
    _, _, moments = cases.filter_inputs(130, 67)
    rec = np.concatenate([rec, moments.reshape(-1, 4)])
    v64, rel64 = d64.variance_of_mean(rec), d64.noise_rel(rec)
    rel, _ = hipmod.noise_host(rec)
    v = host_variance(hipmod, rec)
    bound = cases.variance_bound(rec, v64)
    assert_variance(v, v64, bound, np.zeros(len(rec), bool), "records", absolute=True)
    assert np.array_equal(np.isfinite(rel), np.isfinite(rel64)) and not np.isnan(rel).any()
    known = np.isfinite(rel64)
    err, nb = np.abs(d64.widen(rel)[known] - rel64[known]), cases.noise_bound(rec, v64, rel64, bound)[known]
    pos = np.isfinite(v64) & (v64 > 0)
    print(f"noise_rel: largest error / bound {float((err / np.maximum(nb, 1e-300)).max()):.3f}; relative error of the variance up to "
          f"{float(np.max(np.abs(v[pos] - v64[pos]) / v64[pos])):.3e}")
    assert (err <= nb).all()


@pytest.mark.parametrize("w,h", SIZES)
def test_hostile_inputs_pass_through_are_skipped_and_stay_unknown(hipmod, w, h):
    """NaN, infinities, 3e38, negative and denormal colours; records with non-finite or inconsistent sums; zero normals.  Only the documented rules: a centre
    that is not finite comes back bit for bit; a tap that is not finite is skipped (a finite neighbour of one still agrees with float64, unless a value
    beyond 1e18 is in its reach, whose squares leave the f32 range); an unknown variance is +inf and no variance is NaN; nothing finite becomes NaN."""
    img, g, moments = cases.filter_inputs(w, h, hostile=True)
    bad = ~np.isfinite(img).all(axis=-1)
    with np.errstate(invalid="ignore"):
        huge = (np.abs(img) > 1e18).any(axis=-1)
    near_huge = np.zeros((h, w), bool)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            near_huge |= d64.shifted(huge, dy, dx, False)
    near_bad = np.zeros((h, w), bool)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            near_bad |= d64.shifted(bad, dy, dx, False)
    assert bad.sum() > 5 and (near_bad & ~bad & ~near_huge).sum() > 20
    unknown = ~np.isfinite(d64.variance_of_mean(moments))
    for sv in (0.0, 4.0):
        p = hipmod.denoise_var_params(iterations=1, demodulate=0, sigma_color=1.0, sigma_variance=sv)
        got, got_v = hipmod.denoise_variance_host(img, *planes(g), moments, p, 0)
        plain = hipmod.denoise_host(img, *planes(g), p.base, 0)
        want, want_v, flagged = d64.filter_variance(img, g, moments, p, 0)
        for out in (got, plain) if sv == 0.0 else (got,):
            assert np.array_equal(out[bad].view(np.uint32), img[bad].view(np.uint32))                      # passes through
            assert not np.isnan(out[~bad]).any()                                                          # nothing finite becomes NaN
            look = near_bad & ~bad & ~near_huge & ~flagged
            assert rel_diff(out, want)[look].max() <= cases.VARIANCE_TOL                                  # skipped, not averaged in
        assert not np.isnan(got_v).any() and np.isinf(got_v[unknown]).all() and np.array_equal(np.isinf(got_v), unknown)
        assert np.array_equal(np.isinf(want_v), unknown)


# ---- temporal reuse ------------------------------------------------------------------------------------------------------------------------------------

def run_temporal(hipmod, img, g, moments, cam, prev, p, op=0):
    return hipmod.denoise_temporal_host(img, *planes(g), moments, cam, prev, p, op)


@pytest.mark.parametrize("w,h", SIZES)
def test_temporal_reuse_against_float64(rpt, hipmod, oracle, w, h):
    """A -> a moved B, A -> A (the identity path), the all-sky pair (near, and 3000 units apart), a previous camera that looked the other way; max_history 8 / 32 /
    inf, plane_max 0.5 / 2 / inf.  Colour, T, records, reuse decisions and the count end to end; the variance end to end without passes, with passes against
    float64 passes run from the host hook's own blend (cases.passes_from_the_blend)."""
    worst = {"colour": 0.0, "T": 0.0, "records": 0.0}
    for name, it, dem, sv, cap, plane, op in cases.TEMPORAL_CASES:
        what = f"{w}x{h} {name} iterations {it} demodulate {dem} sigma_variance {sv} max_history {cap} plane_max {plane} op {op}"
        img, g, moments, cam, prev = cases.temporal_inputs(rpt, oracle, w, h, name)
        p = hipmod.temporal_params(iterations=it, demodulate=dem, sigma_variance=sv, max_history=cap, normal_min=0.9, plane_max=plane)
        got = run_temporal(hipmod, img, g, moments, cam, prev, p, op)
        watch = cases.VarianceBound(moments)
        want = d64.temporal(img, g, moments, cam, prev, p, op, watch=watch)
        want["bound"] = watch.of(want["variance"])
        figures = assert_temporal(got, want, moments, it, what, after=cases.passes_from_the_blend(got["records"], got["history"], moments, g, p, op) if it else None)
        assert (want["pixels_with_history"] == 0) == (name == "behind") and want["pixels_with_history"] < w * h, what
        worst = {k: max(worst[k], figures[k]) for k in worst}
    print(f"{w}x{h}: largest relative differences {worst} (tolerances {cases.TEMPORAL_TOL:.3e}, {cases.TEMPORAL_T_TOL:.3e}, {cases.TEMPORAL_RECORDS_TOL:.3e})")


def test_temporal_hostile_inputs(rpt, hipmod, oracle):
    """hostile colours, records and zero normals in both views (history records as the library writes them: N = 0 where the colour is not finite): a current
    mean that is not finite passes through and leaves N = 0; nothing finite becomes NaN; no variance is NaN; reuse decisions still those of float64.
    One exception, which csrc/k_temporal.h states: a record whose COUNT m.z is NaN or infinite (no render produces one; a caller's moments image could) makes T
    and with it the blended colour NaN — it leaves N = 0 behind, so it goes no further; that is asserted here."""
    w, h = 37, 23
    img, g, moments, cam, prev = cases.temporal_inputs(rpt, oracle, w, h, "A->B", hostile=True)
    rec = prev["records"]
    rec[~np.isfinite(rec[..., :3]).all(axis=-1) | ~np.isfinite(rec[..., 3]), 3] = 0
    rec[..., 4:] = np.where(np.isfinite(rec[..., 4:]), rec[..., 4:], F(0.5))
    p = hipmod.temporal_params(iterations=0, demodulate=0, max_history=32.0, normal_min=0.9, plane_max=2.0)
    got = run_temporal(hipmod, img, g, moments, cam, prev, p, 0)
    want = d64.temporal(img, g, moments, cam, prev, p, 0)
    bad = ~np.isfinite(img).all(axis=-1)
    assert bad.sum() > 5
    assert np.array_equal(got["rgb"][bad].view(np.uint32), img[bad].view(np.uint32)) and (got["records"][bad][:, 3] == 0).all()
    counted = np.isfinite(moments[..., 2])
    assert (~counted).sum() > 5 and (got["records"][~counted & want["reused"]][:, 3] == 0).all()
    assert not np.isnan(got["rgb"][~bad & counted]).any() and not np.isnan(got["variance"]).any()
    near = want["margin"] < DELTA
    with np.errstate(invalid="ignore"):
        assert np.array_equal((got["history"] > moments[..., 2])[~near & ~bad & counted], want["reused"][~near & ~bad & counted])
    assert not want["reused"][bad].any()
    # a record whose m.x or m.y is not finite adds 0 to the blended moments (its count still counts): mu1, mu2 of the new history against float64
    sums_bad = ~(np.isfinite(moments[..., 0]) & np.isfinite(moments[..., 1]))
    with np.errstate(invalid="ignore"):
        look = sums_bad & counted & ~bad & ~near & want["reused"] & (np.abs(want["records"][..., 4:]) < 1e30).all(axis=-1)
    assert look.sum() > 5
    assert np.isfinite(got["records"][look][:, 4:]).all()
    assert rel_diff(got["records"][..., 4:], want["records"][..., 4:])[look].max() <= cases.TEMPORAL_RECORDS_TOL


def test_the_plane_test_counts_at_its_threshold(rpt, hipmod, oracle):
    """the same camera twice (the one tap is the pixel itself), the previous view's surface 1.96 footprints off the centre's tangent plane in one column and 2.04
    in another, plane_max = 2 (and 0.5 x, with plane_max = 1): the first column reuses its history, the hits of the second do not — on the host hook and in
    float64.  (The room's own taps lie on the plane or far off it, where any threshold gives the same answer.)"""
    import test_denoise_temporal as tt
    w, h = 37, 23
    cam = tt.camera(rpt, w, h)
    g = tt.room(cam, oracle)
    img, m = tt.flat_inputs(w, h, 2, 0.5)
    rec = tt.flat_records(w, h, 4.0, 0.2, 0.25, 0.1)
    hits = g["kind"] != 0
    assert hits[:, 10].any() and hits[:, 20].any()
    for plane_max in (2.0, 1.0):
        other = {k: v.copy() for k, v in g.items()}
        for column, footprints in ((10, 0.98 * plane_max), (20, 1.02 * plane_max)):
            other["position"][:, column] = g["position"][:, column] + g["normal"][:, column] * (F(footprints) * F(2.0 / w) * g["depth"][:, column])[:, None]
        p = hipmod.temporal_params(iterations=0, max_history=32.0, normal_min=0.9, plane_max=plane_max)
        prev = tt.previous_of(cam, other, rec)
        got = run_temporal(hipmod, img, g, m, cam, prev, p)
        want = d64.temporal(img, g, m, cam, prev, p)
        expected = np.ones((h, w), bool)
        expected[:, 20] = ~hits[:, 20]
        assert (want["margin"][hits[:, 10], 10] >= DELTA).all() and (want["margin"][hits[:, 20], 20] >= DELTA).all()
        assert np.array_equal(want["reused"], expected), plane_max
        assert np.array_equal(got["history"] > 2, expected), plane_max


# ---- the reprojection against the geometry alone ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["DarkCornell", "VeachMIS"])
def test_a_views_own_hits_project_onto_their_own_pixels(rpt, oracle, world, scene):
    """every hit pixel q of a view's guides, projected through that view's camera, lands on (q.x, q.y): within the 7.4e-5 pixels that
    tests/test_denoise_temporal.py documents for the f32 side (here the error is that of the f32 guides: position and the library's f32 rotation)"""
    w, h = 130, 67
    for changes in ({}, dict(cam_position=(0.3, 0.1, -0.2, 0.0), cam_rotation=(0.05, -0.12, 0.0, 0.0))):
        cfg = rpt.default_config(w, h)
        for k, v in changes.items():
            for j in range(3):
                getattr(cfg, k)[j] += v[j]
        g = denoise_ref.guides(world(scene), cfg, oracle)
        hit = g["kind"] != 0
        assert hit.sum() > w * h // 3
        fx, fy, usable, _ = d64.reproject(g["position"], g["kind"], cfg, cfg, w, h)
        ys, xs = np.mgrid[0:h, 0:w]
        worst = max(np.abs(fx - xs)[hit].max(), np.abs(fy - ys)[hit].max())
        print(f"{scene} {changes}: largest round-trip error {worst:.3e} pixels (bound 7.4e-5)")
        assert usable[hit].all() and worst <= 7.4e-5


def test_a_static_affine_history_comes_back_at_the_centres_own_position(rpt, hipmod, oracle):
    """The history colour is an affine function f of the world position on the room's wall (z = 6).  After A -> B a wall pixel p whose four taps are wall
    pixels must reuse f(x_p), up to the second-order term of bilinear interpolation: seen from A the wall's positions are x(s) = o + (6 - o.z) d(s) / d.z(s),
    d affine in the screen position s, so every channel of f(x(s)) is a ratio g = A(s) / B(s) of affine functions, with g_xx = 2 B_x (A B_x - A_x B) / B^3
    and g_yy alike.  A B_x - A_x B does not depend on x and 1 / B^3 is convex, so over a cell |g_xx| is largest at a corner; bilinear interpolation over a
    unit cell errs by at most (max |g_xx| + max |g_yy|) / 8.  Beside it only what the f32 side can contribute: the documented 7.4e-5 pixels of its projection
    times the gradient of g (g_x = (A_x B - A B_x) / B^2, largest at a corner for the same reasons), and sixteen roundoffs of the value (the stored history, four
    weights, four products and sums, the quotient by Wt, the blend's product and quotient)."""
    import test_denoise_temporal as tt
    for w, h in SIZES:
        cam_b, cam_a = tt.camera(rpt, w, h), tt.camera(rpt, w, h, **cases.MOVED)      # the PREVIOUS view is the pitched and yawed one: seen from it the wall is not affine
        g_a, g_b = tt.room(cam_a, oracle, 1), tt.room(cam_b, oracle, 2)
        c0, c = np.array([0.8, 1.1, 0.6]), np.array([[0.07, -0.05, 0.0], [0.02, 0.09, 0.0], [-0.06, 0.03, 0.0]])      # f(x) = c0 + c x, per channel; positive over the wall
        f = lambda x: c0 + d64.widen(x) @ c.T
        rec = np.zeros((h, w, 6), F)
        rec[..., :3], rec[..., 3], rec[..., 4], rec[..., 5] = f(g_a["position"]), 4.0, 0.5, 0.3
        img, moments = np.zeros((h, w, 3), F), np.zeros((h, w, 4), F)                                           # no current samples: the blend is the history alone
        p = hipmod.temporal_params(iterations=0, demodulate=0, max_history=32.0, normal_min=0.9, plane_max=2.0)
        prev = tt.previous_of(cam_a, g_a, rec)
        got = run_temporal(hipmod, img, g_b, moments, cam_b, prev, p, 0)
        want = d64.temporal(img, g_b, moments, cam_b, prev, p, 0)
        # the pixels: wall surface in B whose four taps in A are wall surface too
        wall_a = (g_a["kind"] == 1) & (g_a["normal"][..., 2] == -1)
        fx, fy, usable, _ = d64.reproject(g_b["position"], g_b["kind"], cam_b, cam_a, w, h)
        x0, y0 = np.floor(np.where(usable, fx, 0)).astype(int), np.floor(np.where(usable, fy, 0)).astype(int)
        ok = usable & (g_b["kind"] == 1) & (g_b["normal"][..., 2] == -1) & (x0 >= 0) & (y0 >= 0) & (x0 + 1 < w) & (y0 + 1 < h)
        x0, y0 = np.clip(x0, 0, w - 2), np.clip(y0, 0, h - 2)
        ok &= wall_a[y0, x0] & wall_a[y0, x0 + 1] & wall_a[y0 + 1, x0] & wall_a[y0 + 1, x0 + 1] & (want["margin"] >= DELTA)
        assert ok.sum() > w * h // 4 and want["reused"][ok].all()
        # the second-order term, from A's camera: d(s) = R (ux, uy, 1), ux = 2 sx / W - 1, uy = (1 - 2 sy / H) H / W
        R, o = d64.camera_rotation(cam_a), d64.camera_position(cam_a)
        d_x, d_y = R[:, 0] * (2.0 / w), R[:, 1] * (-2.0 / w)                                                   # the gradients of d in pixels
        bound, slope = np.zeros((h, w, 3)), np.zeros((h, w, 3))
        for cy in (0, 1):
            for cx in (0, 1):
                sx, sy = x0 + cx + 0.5, y0 + cy + 0.5
                d = (sx[..., None] * d_x + sy[..., None] * d_y) + R @ np.array([-1.0, h / w, 1.0])
                B = d[..., 2]
                for ch in range(3):
                    A, scale = d @ c[ch], (6.0 - o[2])
                    gxx = 2 * d_x[2] * (A * d_x[2] - (d_x @ c[ch]) * B) / B ** 3
                    gyy = 2 * d_y[2] * (A * d_y[2] - (d_y @ c[ch]) * B) / B ** 3
                    bound[..., ch] = np.maximum(bound[..., ch], scale * (np.abs(gxx) + np.abs(gyy)) / 8)
                    gx, gy = ((d_x @ c[ch]) * B - A * d_x[2]) / B ** 2, ((d_y @ c[ch]) * B - A * d_y[2]) / B ** 2
                    slope[..., ch] = np.maximum(slope[..., ch], scale * (np.abs(gx) + np.abs(gy)))
        truth = f(g_b["position"])
        for name, e in (("host hook", got["records"][..., :3]), ("float64", want["records"][..., :3])):
            err = np.abs(d64.widen(e) - truth)
            allowed = bound + 7.4e-5 * slope + 16 * 2.0 ** -24 * np.abs(truth)
            step = np.abs(np.diff(truth, axis=1))[ok[:, 1:] & ok[:, :-1]]
            print(f"{w}x{h} {name}: largest error {err[ok].max():.3e}, largest allowance {allowed[ok].max():.3e} (second-order term {bound[ok].max():.3e}), "
                  f"a pixel's step of f: median {np.median(step):.3e}, largest {step.max():.3e}")
            assert (err[ok] <= allowed[ok]).all(), name
            assert 0 < bound[ok].max() and allowed[ok].max() < 0.05 * np.median(step)                           # (the allowance is far below one pixel's step)


# ---- the moments against the samples ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,nee", [("DarkCornell", 0), ("VeachMIS", 1)])
def test_the_moments_record_against_the_samples_in_float64(rpt, hipmod, oracle, world, scene, nee):
    """float64 variance of the mean and relative standard error straight from the oracle's per-sample radiances, against mo_add's f32 record through the host
    hooks, after 2, 3, 16 and 64 samples at 64 x 48: the bound of a given record with (n + c) in place of c, for the n roundings of each running sum"""
    w, h = 64, 48
    cfg = rpt.default_config(w, h, nee=nee)
    bank = SampleBank(oracle, cfg, world(scene), rpt.blue_noise_seeds(w, h))
    for n in (2, 3, 16, 64):
        rec = bank.moments(n)
        m64 = d64.moments_of_samples(np.stack(bank.radiance[:n]))
        v64, rel64 = d64.variance_of_mean(m64), d64.noise_rel(m64)
        rel, _ = hipmod.noise_host(rec)
        v = host_variance(hipmod, rec)
        assert np.isfinite(v64).all() and (v64 > 0).sum() > 20                     # (DarkCornell without NEE: 40 pixels of 3072 after two samples)
        bound = cases.variance_bound(m64, v64, extra=n)
        assert_variance(v, v64, bound, np.zeros((h, w), bool), f"{scene} nee {nee} n {n}", absolute=True)
        err, nb = np.abs(d64.widen(rel) - rel64), cases.noise_bound(m64, v64, rel64, bound, extra=n)
        print(f"{scene} nee {nee} n {n}: noise_rel, largest error / bound {float((err / np.maximum(nb, 1e-300)).max()):.3f}; {int((v64 == 0).sum())} pixels with zero variance")
        assert np.isfinite(rel).all() and (err <= nb).all()
