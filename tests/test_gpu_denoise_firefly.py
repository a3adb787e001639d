"""The firefly clamp on the device (clamp_scale / clamp_floor / clamp_radius of rpt_denoise_variance and rpt_denoise_temporal; csrc/k_firefly.h
k_dn_prepare_var_clamp, k_dn_temporal_clamp) against the host build of the same header, bit for bit — colour, variance, T — and pixels_clamped against the
host's mask; from the context's own record, a caller's image, per-pixel counts, a gathered image and several ranks; along a temporal path; a planted case
built through the C ABI alone against the numpy prediction; a resumed accumulator; the clamp off; without side effects; and its refusals.

DarkCornell with NEE (walked from LDS) and VeachMIS with NEE at 130 x 67, 8 spp, moments on: partial 64-pixel row segments, a height that is no multiple of
4, and edges of the 64 x 64 tiles of the accumulator's order inside the image — the window of a pixel next to such an edge reads records of another tile."""
import ctypes as C

import numpy as np
import pytest

import firefly_ref
from test_denoise_firefly import garbage, planted

pytestmark = pytest.mark.gpu

W, H, SPP = 130, 67, 8
F = np.float32
SCENES = [("DarkCornell", 1), ("VeachMIS", 1)]
SIGMA = 4.0


def same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.fixture(scope="module")
def r(hipmod):
    """a Renderer of the module's own: it keeps moments on, which the session's renderer must not"""
    r = hipmod.Renderer(0)
    yield r
    r.close()


def begin(r, rpt, world, scene, nee, spp=SPP, cfg=None):
    r.upload_scene(world(scene))
    r.set_config(cfg or rpt.default_config(W, H, nee=nee))
    r.reset(rpt.blue_noise_seeds(W, H))
    r.set_moments(False)
    r.set_moments(True)                                 # (zeroes the record)
    r.temporal_reset()
    if spp:
        r.render(spp)


def inputs(r, moments=None):
    """the device's mean (every pixel by its own count while the counts differ), counts, guides and moments"""
    acc, n = r.read_accum()
    if r.counts_uniform():
        mean, counts = (acc[..., :3] / F(n)).astype(F), np.full(acc.shape[:2], F(n))
    else:
        with np.errstate(all="ignore"):
            mean, counts = np.where(acc[..., 3:] == 0, F(0.0), acc[..., :3] / acc[..., 3:]).astype(F), acc[..., 3].copy()
    return mean, counts, r.guides(), r.read_moments() if moments is None else moments


def host_mask(hipmod, r, vp, moments=None):
    mean, counts, g, m = inputs(r, moments)
    dem = vp.base.iterations != 0 and vp.base.demodulate != 0
    return hipmod.firefly_host(mean, g["albedo"], g["kind"], m, counts, 0, vp.clamp_scale, vp.clamp_floor, vp.clamp_radius, dem)[2] != 0


def check_variance(hipmod, r, p, op, what, moments=None, **source):
    """the device call against the host hook (which takes count = m.z: the tests below say where that is the accumulator's count); returns pixels_clamped"""
    mean, counts, g, m = inputs(r, moments)
    assert np.array_equal(counts, m[..., 2]), what
    rgb, var, rep = r.denoise_variance(params=p, tonemap_op=op, with_report=True, **source)
    want_rgb, want_var = hipmod.denoise_variance_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], m, p, op)
    assert same_bits(rgb, want_rgb), what + ": colour"
    assert same_bits(var, want_var), what + ": variance"
    assert rep["pixels_clamped"] == int(host_mask(hipmod, r, p, moments).sum()), what + ": pixels_clamped"
    return rep["pixels_clamped"]


@pytest.mark.parametrize("scene,nee", SCENES)
def test_device_equals_the_host_hook_bitwise(r, rpt, hipmod, world, scene, nee):
    """radius 1 / 2 / 3, demodulation on and off, resolve only; the context's own record and a caller's image"""
    begin(r, rpt, world, scene, nee)
    counts = {}
    for radius in (1, 2, 3):
        for it, dem, op in ((2, 1, 0), (1, 0, 3), (0, 1, 2)):
            p = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_variance=SIGMA, clamp_scale=2.0, clamp_radius=radius)
            what = f"{scene} radius {radius} iterations {it} demodulate {dem}"
            counts[radius, it] = check_variance(hipmod, r, p, op, what)
            own = r.denoise_variance(params=p, tonemap_op=op, with_report=True)
            given = r.denoise_variance(moments=r.read_moments(), params=p, tonemap_op=op, with_report=True)
            assert same_bits(given[0], own[0]) and same_bits(given[1], own[1]) and given[2]["pixels_clamped"] == own[2]["pixels_clamped"], what + ": caller's image"
    print(f"{scene}: pixels_clamped {counts}")
    assert all(0 < v <= W * H // 8 for v in counts.values())
    p = hipmod.denoise_var_params(iterations=2, sigma_variance=SIGMA, clamp_scale=1.0, clamp_floor=0.05, clamp_radius=1)       # scale 1: every local maximum above the floor
    assert check_variance(hipmod, r, p, 0, scene + " scale 1") > counts[1, 2]
    off = hipmod.denoise_var_params(iterations=2, sigma_variance=SIGMA)
    assert not same_bits(r.denoise_variance(params=off)[0], r.denoise_variance(params=hipmod.denoise_var_params(iterations=2, sigma_variance=SIGMA, clamp_scale=2.0))[0])


def test_with_per_pixel_counts(r, rpt, hipmod, world):
    """after rpt_render_pixels on a checkerboard: every pixel's mean and count_p are its own .w, which its record's m.z equals"""
    begin(r, rpt, world, "DarkCornell", 1)
    yy, xx = np.mgrid[0:H, 0:W]
    r.render_pixels((yy + xx) % 2 == 0, 5)
    assert not r.counts_uniform() and set(np.unique(r.read_moments()[..., 2])) == {8.0, 13.0}
    for radius, it, dem in ((1, 2, 1), (3, 1, 0)):
        p = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_variance=SIGMA, clamp_scale=2.0, clamp_radius=radius)
        assert check_variance(hipmod, r, p, 0, f"checkerboard radius {radius}") > 0


def test_gathered_and_several_ranks(r, rpt, hipmod, world):
    """RPT_DENOISE_GATHERED after rpt_comm_init_local with the moments as an image, and 2 and 3 ranks through rpt_multi_*: the one context's bytes and count"""
    begin(r, rpt, world, "DarkCornell", 1)
    p = hipmod.denoise_var_params(iterations=2, sigma_variance=SIGMA, clamp_scale=2.0, clamp_radius=2)
    tp = hipmod.temporal_params(iterations=2, sigma_variance=SIGMA, clamp_scale=2.0, clamp_radius=2)
    one = r.denoise_variance(params=p, tonemap_op=3, with_report=True)
    one_t = r.denoise_temporal(params=tp, tonemap_op=3, with_report=True)
    assert one[2]["pixels_clamped"] > 0 and one_t[3]["pixels_clamped"] == one[2]["pixels_clamped"]
    g = hipmod.Renderer(0)
    try:
        begin(g, rpt, world, "DarkCornell", 1, spp=0)
        g.comm_init_local()
        g.reset(rpt.blue_noise_seeds(W, H))
        g.render(SPP)
        g.gather_async()
        got = g.denoise_variance(source=hipmod.DENOISE_GATHERED, moments=g.read_moments(), params=p, tonemap_op=3, with_report=True)
        assert same_bits(got[0], one[0]) and same_bits(got[1], one[1]) and got[2]["pixels_clamped"] == one[2]["pixels_clamped"]
        g.gather_async()
        got = g.denoise_temporal(source=hipmod.DENOISE_GATHERED, moments=g.read_moments(), params=tp, tonemap_op=3, with_report=True)
        assert all(same_bits(x, y) for x, y in zip(got[:3], one_t[:3])) and got[3]["pixels_clamped"] == one[2]["pixels_clamped"]
    finally:
        g.close()
    for ranks in (2, 3):
        m = hipmod.MultiRenderer([0] * ranks, allow_shared_device=True)
        try:
            m.upload_scene(world("DarkCornell"))
            m.set_config(rpt.default_config(W, H, nee=1))
            m.reset(rpt.blue_noise_seeds(W, H))
            m.set_moments(True)
            m.render(SPP)
            many = m.denoise_variance(params=p, tonemap_op=3, with_report=True)
            assert same_bits(many[0], one[0]) and same_bits(many[1], one[1]) and many[2]["pixels_clamped"] == one[2]["pixels_clamped"], ranks
            many = m.denoise_temporal(params=tp, tonemap_op=3, with_report=True)
            assert all(same_bits(x, y) for x, y in zip(many[:3], one_t[:3])) and many[3]["pixels_clamped"] == one[2]["pixels_clamped"], ranks
        finally:
            m.close()


@pytest.mark.parametrize("scene,nee", SCENES)
def test_along_the_temporal_path(r, rpt, hipmod, world, scene, nee):
    """A -> B -> B with the clamp on: the device against the host hook chained through its own records, in which a clamped pixel's history is c' and not c"""
    cam_a = rpt.default_config(W, H, nee=nee)
    cam_b = cam_a.copy()
    cam_b.cam_position[0] += 0.3
    cam_b.cam_rotation[1] += 0.1
    p = hipmod.temporal_params(iterations=2, demodulate=1, sigma_variance=SIGMA, max_history=32.0, normal_min=0.9, plane_max=2.0, clamp_scale=2.0, clamp_radius=2)
    off = hipmod.temporal_params(iterations=2, demodulate=1, sigma_variance=SIGMA, max_history=32.0, normal_min=0.9, plane_max=2.0)

    def step(cam, previous, previous_off, what):
        mean, counts, g, m = inputs(r)
        assert np.array_equal(counts, m[..., 2])
        run = lambda prm, prev: hipmod.denoise_temporal_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], m, cam, prev, prm, 0)
        want, plain = run(p, previous), run(off, previous_off)
        rgb, var, hist, rep = r.denoise_temporal(params=p, with_report=True)
        assert same_bits(rgb, want["rgb"]) and same_bits(var, want["variance"]) and same_bits(hist, want["history"]), what
        mask = host_mask(hipmod, r, p.filter)
        assert rep["pixels_with_history"] == want["pixels_with_history"] and rep["pixels_clamped"] == int(mask.sum()) > 0, what
        nxt = lambda out: {"camera": cam.copy(), "normal": g["normal"], "position": g["position"], "kind": g["kind"], "records": out["records"]}
        return nxt(want), nxt(plain), mask, rep

    begin(r, rpt, world, scene, nee, cfg=cam_a)
    a, a_off, mask_a, rep = step(cam_a, None, None, scene + " A")
    assert rep["history_state"] == hipmod.HISTORY_NONE
    assert (a["records"][mask_a][:, :3] < a_off["records"][mask_a][:, :3]).any() and same_bits(a["records"][~mask_a], a_off["records"][~mask_a])     # c', not c
    r.set_config(cam_b)
    r.reset(rpt.blue_noise_seeds(W, H))
    r.render(SPP)
    b, _, _, rep = step(cam_b, a, a_off, scene + " A->B")
    assert rep["history_state"] == hipmod.HISTORY_USED and 0 < rep["pixels_with_history"] < W * H
    r.render(SPP)
    step(cam_b, a, a_off, scene + " A->B->B")


def test_a_planted_case_through_the_c_abi(r, rpt, hipmod, world, oracle):
    """rpt_reset with accum_init and samples_init = n plus a caller's moments image with m.z = n and known spikes: nothing rendered; the output is the numpy
    prediction (tests/firefly_ref.py), and pixels_clamped its mask"""
    begin(r, rpt, world, "DarkCornell", 1, spp=0)
    mean, m, spike = planted(W, H, 77)
    acc = np.concatenate([(mean * F(SPP)).astype(F), np.full((H, W, 1), F(SPP))], -1)
    r.reset(rpt.blue_noise_seeds(W, H), acc, SPP)
    got_acc, n = r.read_accum()
    assert n == SPP and same_bits(got_acc, acc)
    mean = (acc[..., :3] / F(SPP)).astype(F)
    g = r.guides()
    for it, dem, radius, op in ((0, 0, 2, 0), (2, 1, 1, 0), (1, 0, 3, 3)):
        p = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_variance=SIGMA, clamp_scale=2.0, clamp_radius=radius)
        rgb, var, rep = r.denoise_variance(moments=m, params=p, tonemap_op=op, with_report=True)
        want_rgb, want_var, mask = firefly_ref.denoise_variance(mean, g, m, p, op, oracle, counts=SPP)
        what = f"iterations {it} demodulate {dem} radius {radius}"
        assert same_bits(rgb, want_rgb) and same_bits(var, want_var), what
        assert rep["pixels_clamped"] == int(mask.sum()) > 0, what
        if not dem:
            assert (mask & spike).sum() > 0.5 * mask.sum(), what
        if it == 0:
            c1 = firefly_ref.clamp(mean, g["albedo"], g["kind"], m, SPP, 2.0, 0.0, radius, False)[0]
            assert same_bits(rgb, c1) and (rgb[mask] < mean[mask]).any() and same_bits(rgb[~mask], mean[~mask])
    tp = hipmod.temporal_params(iterations=0, clamp_scale=2.0, clamp_radius=2)
    rgb, var, hist, rep = r.denoise_temporal(moments=m, params=tp, with_report=True)
    c1, m1, mask = firefly_ref.clamp(mean, g["albedo"], g["kind"], m, SPP, 2.0, 0.0, 2, False)
    assert same_bits(rgb, c1) and rep["pixels_clamped"] == int(mask.sum()) and same_bits(hist, m[..., 2])
    # a record that counts differently from the accumulator is left alone: pixel by pixel
    m2 = m.copy()
    m2[::2, :, 2] = SPP + 1
    p = hipmod.denoise_var_params(iterations=0, clamp_scale=2.0, clamp_radius=2)
    rgb, _, rep = r.denoise_variance(moments=m2, params=p, with_report=True)
    want = firefly_ref.clamp(mean, g["albedo"], g["kind"], m2, SPP, 2.0, 0.0, 2, False)
    assert same_bits(rgb, want[0]) and rep["pixels_clamped"] == int(want[2].sum()) > 0 and not want[2][::2].any()


def test_a_resumed_accumulator_clamps_nothing(r, rpt, hipmod, world):
    """rpt_reset with accum_init resumes the accumulator and not the moments: m.z counts the samples since, count_p all of them"""
    begin(r, rpt, world, "DarkCornell", 1)
    acc, n = r.read_accum()
    r.reset(r.read_rng(), acc, n)
    r.render(SPP)
    assert r.read_accum()[1] == 2 * SPP and (r.read_moments()[..., 2] == SPP).all()
    for radius in (1, 3):
        on = hipmod.denoise_var_params(iterations=2, sigma_variance=SIGMA, clamp_scale=1.0, clamp_radius=radius)
        off = hipmod.denoise_var_params(iterations=2, sigma_variance=SIGMA)
        a, b = r.denoise_variance(params=on, with_report=True), r.denoise_variance(params=off, with_report=True)
        assert a[2]["pixels_clamped"] == 0 and same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    t = r.denoise_temporal(params=hipmod.temporal_params(iterations=2, clamp_scale=1.0, clamp_radius=2), with_report=True)
    assert t[3]["pixels_clamped"] == 0


@pytest.mark.parametrize("scene,nee", SCENES)
def test_the_clamp_off_is_the_call_without_the_fields(r, rpt, hipmod, world, scene, nee):
    """clamp_scale 0: the other two words are not read, pixels_clamped is 0, and the bytes are those of the host hook, of rpt_denoise where the term is off too,
    and of the same call with the words set to anything"""
    begin(r, rpt, world, scene, nee)
    for it, dem, op in ((2, 1, 3), (0, 1, 1), (1, 0, 0)):
        off = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_variance=SIGMA)
        a, b = r.denoise_variance(params=off, tonemap_op=op, with_report=True), r.denoise_variance(params=garbage(off), tonemap_op=op, with_report=True)
        assert off.clamp_scale == 0 and a[2]["pixels_clamped"] == b[2]["pixels_clamped"] == 0 and same_bits(a[0], b[0]) and same_bits(a[1], b[1])
        assert check_variance(hipmod, r, off, op, f"{scene} off") == 0
        plain = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_variance=0.0)
        assert same_bits(r.denoise_variance(params=garbage(plain), tonemap_op=op)[0], r.denoise(params=plain.base, tonemap_op=op))
        toff = hipmod.temporal_params(iterations=it, demodulate=dem, sigma_variance=SIGMA)
        r.temporal_reset()
        ta = r.denoise_temporal(params=toff, tonemap_op=op, with_report=True)
        r.temporal_reset()
        tb = r.denoise_temporal(params=garbage(toff), tonemap_op=op, with_report=True)
        assert ta[3]["pixels_clamped"] == tb[3]["pixels_clamped"] == 0 and all(same_bits(x, y) for x, y in zip(ta[:3], tb[:3]))
        assert same_bits(ta[0], a[0]) and same_bits(ta[1], a[1])                          # no history: rpt_denoise_variance's bytes


def test_no_side_effects(r, rpt, hipmod, world):
    """accumulator, rng, moments, rpt_stats, the cached guides, the shadow mode and the rpt_denoise output are the same before and after"""
    begin(r, rpt, world, "VeachMIS", 1)
    state = lambda: (r.read_accum(), r.read_rng(), r.read_moments(), {k: v for k, v in r.stats().items() if k not in ("render_ms", "kernel_ms", "kernel_launches")}, r.denoise())
    (acc0, n0), rng0, mom0, stats0, den0 = state()
    mode, guides0 = r.shadow_mode(), r.guides()
    p = hipmod.denoise_var_params(iterations=3, sigma_variance=SIGMA, clamp_scale=2.0, clamp_radius=3)
    _, _, rep = r.denoise_variance(params=p, with_report=True)
    assert rep["guides_rebuilt"] == 0 and rep["device_ms"] > 0 and rep["pixels_clamped"] > 0
    r.denoise_variance(moments=mom0 * F(2.0), params=p)
    trep = r.denoise_temporal(params=hipmod.temporal_params(clamp_scale=2.0, clamp_radius=1), with_report=True)[3]
    assert trep["pixels_clamped"] > 0
    (acc1, n1), rng1, mom1, stats1, den1 = state()
    assert n0 == n1 and same_bits(acc0, acc1) and np.array_equal(rng0, rng1) and same_bits(mom0, mom1) and stats0 == stats1 and same_bits(den0, den1)
    assert r.shadow_mode() == mode and r.moments_on() and all(same_bits(guides0[k].view(F), r.guides()[k].view(F)) for k in guides0)
    assert r.denoise(with_report=True)[1]["pixels_clamped"] == 0                          # plain rpt_denoise has no record and no clamp
    r.render(SPP)
    assert r.read_accum()[1] == 2 * SPP


def test_refusals_leave_the_context_usable(r, rpt, hipmod, world):
    begin(r, rpt, world, "DarkCornell", 1)
    p = hipmod.denoise_var_params(iterations=2, sigma_variance=SIGMA, clamp_scale=2.0, clamp_radius=2)
    good = r.denoise_variance(params=p, with_report=True)
    bad = [dict(clamp_scale=-1.0), dict(clamp_scale=float("nan")), dict(clamp_scale=float("inf")), dict(clamp_scale=1.0, clamp_floor=-0.5),
           dict(clamp_scale=1.0, clamp_floor=float("nan")), dict(clamp_scale=1.0, clamp_floor=float("inf")), dict(clamp_scale=1.0, clamp_radius=0),
           dict(clamp_scale=1.0, clamp_radius=4)]
    for fields in bad:
        for call in (lambda: r.denoise_variance(params=hipmod.denoise_var_params(**fields)), lambda: r.denoise_temporal(params=hipmod.temporal_params(**fields))):
            with pytest.raises(hipmod.RptError) as e:
                call()
            assert e.value.code == -1 and "clamp" in str(e.value), fields
        again = r.denoise_variance(params=p, with_report=True)
        assert same_bits(again[0], good[0]) and same_bits(again[1], good[1]) and again[2]["pixels_clamped"] == good[2]["pixels_clamped"], fields
    r.denoise_variance(params=hipmod.denoise_var_params(clamp_floor=-1.0, clamp_radius=99))          # the clamp off: the two words are not read
    r.render(SPP)
    assert r.read_accum()[1] == 2 * SPP
