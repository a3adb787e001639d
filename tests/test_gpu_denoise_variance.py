"""The variance-guided filter on the device (rpt_denoise_variance, rpt_multi_denoise_variance; csrc/k_denoise.h k_dn_pass_var, rpt_denoise.hip
k_dn_prepare_var) against the host build of the same headers, bit for bit, colour and variance; with per-pixel counts; with one measured pixel; against
rpt_denoise with the term off; with a caller's moments image; without side effects; over several ranks; and its refusals.

DarkCornell (walked from LDS) and VeachMIS with NEE at 130 x 67, 8 spp, moments on: partial 64-pixel row segments, a height that is no multiple of 4, and
edges of the 64 x 64 tiles of the accumulator's order inside the image."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP = 130, 67, 8
F = np.float32
SCENES = [("DarkCornell", 0), ("VeachMIS", 1)]
SIGMA = 4.0                                             # the term is on in every case that does not say otherwise (the shipped default may be 0)


def same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.fixture(scope="module")
def r(hipmod):
    """a Renderer of the module's own: it keeps moments on, which the session's renderer must not"""
    r = hipmod.Renderer(0)
    yield r
    r.close()


def begin(r, rpt, world, scene, nee, spp=SPP):
    r.upload_scene(world(scene))
    r.set_config(rpt.default_config(W, H, nee=nee))
    r.reset(rpt.blue_noise_seeds(W, H))
    r.set_moments(False)
    r.set_moments(True)                                 # (zeroes the record)
    if spp:
        r.render(spp)


def host(hipmod, r, params, op, moments=None):
    """the host hook fed the device's accumulator, guides and moments; every pixel by its own count while the counts differ"""
    acc, n = r.read_accum()
    if r.counts_uniform():
        mean = (acc[..., :3] / F(n)).astype(F)
    else:
        with np.errstate(all="ignore"):
            mean = np.where(acc[..., 3:] == 0, F(0.0), acc[..., :3] / acc[..., 3:]).astype(F)
    g = r.guides()
    return hipmod.denoise_variance_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], r.read_moments() if moments is None else moments, params, op)


def check_against_host(hipmod, r, what, cases=None):
    cases = cases or [(it, dem, op) for it in (1, 2, 6) for dem in (0, 1) for op in (0, 3)]
    for it, dem, op in cases:
        p = hipmod.denoise_var_params(iterations=it, demodulate=dem, sigma_variance=SIGMA)
        rgb, var = r.denoise_variance(params=p, tonemap_op=op)
        want_rgb, want_var = host(hipmod, r, p, op)
        assert same_bits(rgb, want_rgb), f"{what}: colour, iterations {it} demodulate {dem} op {op}"
        assert same_bits(var, want_var), f"{what}: variance, iterations {it} demodulate {dem} op {op}"
    return rgb, var


@pytest.mark.parametrize("scene,nee", SCENES)
def test_device_equals_the_host_hook_bitwise(r, rpt, hipmod, world, scene, nee):
    begin(r, rpt, world, scene, nee)
    rgb, var = check_against_host(hipmod, r, scene)
    assert np.isfinite(var).all() and (var > 0).any()                                   # 8 samples everywhere: every variance is known
    p = hipmod.denoise_var_params(iterations=2, sigma_variance=SIGMA)
    assert not same_bits(r.denoise_variance(params=p)[0], r.denoise(params=p.base))      # (the term does something)
    p0 = hipmod.denoise_var_params(iterations=0)
    rgb, var = r.denoise_variance(params=p0, tonemap_op=2)
    want_rgb, want_var = host(hipmod, r, p0, 2)
    assert same_bits(rgb, r.resolve(2)) and same_bits(rgb, want_rgb) and same_bits(var, want_var)


@pytest.mark.parametrize("scene,nee", SCENES)
def test_with_per_pixel_counts(r, rpt, hipmod, world, scene, nee):
    """after rpt_render_pixels on a checkerboard rpt_counts_uniform is 0: every pixel's mean by its own count, its variance from its own record"""
    begin(r, rpt, world, scene, nee)
    yy, xx = np.mgrid[0:H, 0:W]
    r.render_pixels((yy + xx) % 2 == 0, 5)
    assert not r.counts_uniform()
    m = r.read_moments()
    assert set(np.unique(m[..., 2])) == {8.0, 13.0}
    check_against_host(hipmod, r, scene + " checkerboard", [(1, 1, 0), (2, 0, 3), (6, 1, 3)])


def test_a_single_measured_pixel(r, rpt, hipmod, world):
    """a mask of one pixel on a fresh reset: every other record is unmeasured and every other pixel has .w == 0 (it resolves to 0)"""
    begin(r, rpt, world, "DarkCornell", 0, spp=0)
    mask = np.zeros((H, W), bool)
    mask[33, 64] = True                                                                   # first pixel of a row segment, in the second tile column
    r.render_pixels(mask, SPP)
    m, (acc, _) = r.read_moments(), r.read_accum()
    assert (m[..., 2] != 0).sum() == 1 and m[33, 64, 2] == SPP and (acc[..., 3] != 0).sum() == 1
    rgb, var = check_against_host(hipmod, r, "one pixel", [(1, 0, 0), (2, 1, 3), (6, 1, 0)])
    assert np.isinf(var).sum() == W * H - 1 and np.isfinite(var[33, 64])


@pytest.mark.parametrize("scene,nee", SCENES)
def test_off_equals_plain_and_a_callers_image_equals_the_contexts_own(r, rpt, hipmod, world, scene, nee):
    begin(r, rpt, world, scene, nee)
    for it, dem, op in [(1, 0, 0), (2, 1, 3), (6, 1, 5), (0, 1, 1)]:
        base = dict(iterations=it, demodulate=dem)
        off = r.denoise_variance(params=hipmod.denoise_var_params(sigma_variance=0.0, **base), tonemap_op=op)[0]
        assert same_bits(off, r.denoise(params=hipmod.denoise_params(**base), tonemap_op=op)), f"sigma_variance 0 is rpt_denoise, {base}"
        p = hipmod.denoise_var_params(sigma_variance=SIGMA, **base)
        own = r.denoise_variance(params=p, tonemap_op=op)
        given = r.denoise_variance(moments=r.read_moments(), params=p, tonemap_op=op)
        assert same_bits(given[0], own[0]) and same_bits(given[1], own[1]), f"caller's image, {base}"
    assert same_bits(r.denoise_variance()[0], host(hipmod, r, None, 0)[0])               # params NULL: the defaults


def test_no_side_effects(r, rpt, hipmod, world):
    """accumulator, rng, moments, rpt_stats and the rpt_denoise output are the same before and after; and rendering goes on as if the call had not been"""
    begin(r, rpt, world, "VeachMIS", 1)
    state = lambda: (r.read_accum(), r.read_rng(), r.read_moments(), {k: v for k, v in r.stats().items() if k not in ("render_ms", "kernel_ms", "kernel_launches")}, r.denoise())
    (acc0, n0), rng0, mom0, stats0, den0 = state()
    mode, guides0 = r.shadow_mode(), r.guides()
    p = hipmod.denoise_var_params(iterations=3, sigma_variance=SIGMA)
    _, _, rep = r.denoise_variance(params=p, with_report=True)
    assert rep["guides_rebuilt"] == 0 and rep["device_ms"] > 0                            # (the guides were cached by rpt_denoise, and stay)
    r.denoise_variance(moments=mom0 * F(2.0), params=p)                                   # a caller's image does not replace the context's record
    (acc1, n1), rng1, mom1, stats1, den1 = state()
    assert n0 == n1 and same_bits(acc0, acc1) and np.array_equal(rng0, rng1) and same_bits(mom0, mom1) and stats0 == stats1 and same_bits(den0, den1)
    assert r.shadow_mode() == mode and r.moments_on() and all(same_bits(guides0[k].view(F), r.guides()[k].view(F)) for k in guides0)
    r.render(SPP)
    acc_after, n_after = r.read_accum()
    mom_after = r.read_moments()
    begin(r, rpt, world, "VeachMIS", 1, spp=0)
    r.render(SPP)
    r.render(SPP)
    assert r.read_accum()[1] == n_after == 2 * SPP and same_bits(r.read_accum()[0], acc_after) and same_bits(r.read_moments(), mom_after)


@pytest.mark.parametrize("ranks", [2, 3])
def test_multi_equals_one_context(r, rpt, hipmod, world, ranks):
    begin(r, rpt, world, "DarkCornell", 1)
    p = hipmod.denoise_var_params(iterations=3, sigma_variance=SIGMA)
    one = r.denoise_variance(params=p, tonemap_op=3)
    m = hipmod.MultiRenderer([0] * ranks, allow_shared_device=True)
    try:
        m.upload_scene(world("DarkCornell"))
        m.set_config(rpt.default_config(W, H, nee=1))
        m.reset(rpt.blue_noise_seeds(W, H))
        with pytest.raises(hipmod.RptError) as e:                                         # moments off on the ranks
            m.denoise_variance(params=p)
        assert e.value.code == -1 and "moments are off" in str(e.value)
        m.set_moments(True)
        m.render(SPP)
        many = m.denoise_variance(params=p, tonemap_op=3)
        assert same_bits(many[0], one[0]) and same_bits(many[1], one[1])
        m.render(SPP)                                                                     # still usable
        assert m.read_accum()[1] == 2 * SPP
    finally:
        m.close()


def test_refusals_leave_the_context_usable(r, rpt, hipmod, world):
    begin(r, rpt, world, "DarkCornell", 0)
    p = hipmod.denoise_var_params(iterations=2, sigma_variance=SIGMA)
    good = r.denoise_variance(params=p)
    mom = r.read_moments()

    def refused(call, text):
        with pytest.raises(hipmod.RptError) as e:
            call()
        assert e.value.code == -1 and text in str(e.value), (text, str(e.value))
        again = r.denoise_variance(params=p)                                              # the next valid call succeeds, with the same bytes
        assert same_bits(again[0], good[0]) and same_bits(again[1], good[1]), text

    refused(lambda: r.denoise_variance(source=hipmod.DENOISE_GATHERED, params=p), "not part of the gather")
    refused(lambda: r.denoise_variance(params=hipmod.denoise_var_params(sigma_variance=-0.5)), "sigma_variance")
    refused(lambda: r.denoise_variance(params=hipmod.denoise_var_params(sigma_variance=float("nan"))), "sigma_variance")
    refused(lambda: r.denoise_variance(params=hipmod.denoise_var_params(iterations=7)), "iterations")               # (what rpt_denoise refuses)
    refused(lambda: r.denoise_variance(params=p, tonemap_op=7), "tonemap")
    refused(lambda: r.denoise_variance(source=hipmod.DENOISE_GATHERED, moments=mom, params=p), "gathered image")    # no communicator: no gathered image
    L = hipmod.lib()
    var = np.zeros((H, W), F)
    assert L.rpt_denoise_variance(r._h, 0, None, C.byref(p), 0, None, var.ctypes.data_as(C.c_void_p), None) == -1 and b"out_rgb" in L.rpt_last_error(r._h)
    assert same_bits(r.denoise_variance(params=p)[0], good[0])
    r.set_moments(False)
    with pytest.raises(hipmod.RptError) as e:                                             # moments off with a NULL image
        r.denoise_variance(params=p)
    assert e.value.code == -1 and "moments are off" in str(e.value)
    given = r.denoise_variance(moments=mom, params=p)                                     # ... but a caller's image still serves
    assert same_bits(given[0], good[0]) and same_bits(given[1], good[1])
    r.render(SPP)
    assert r.read_accum()[1] == 2 * SPP
