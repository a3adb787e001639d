"""Temporal reuse on the device (rpt_denoise_temporal, rpt_temporal_reset, rpt_multi_denoise_temporal; csrc/k_temporal.h k_dn_temporal) against the host build of
the same header, bit for bit — colour, variance and the blended count T — over a path of views: A alone, A -> B, a second call in B's epoch after more
samples, and back to A; the first call against rpt_denoise_variance; with per-pixel counts; with a caller's moments image; on a gathered image; over
several ranks; what drops the history; without side effects; and its refusals.

DarkCornell (walked from LDS) and VeachMIS with NEE at 130 x 67, 8 spp per view, moments on.  View B is view A moved 0.3 sideways and yawed 0.1: with the host
hook on the oracle's guides 7082 (DarkCornell) and 7528 (VeachMIS) of the 8710 pixels find history there, the others do not."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP = 130, 67, 8
F = np.float32
SCENES = [("DarkCornell", 0), ("VeachMIS", 1)]
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


def views(rpt, nee, w=W, h=H):
    a = rpt.default_config(w, h, nee=nee)
    b = a.copy()
    b.cam_position[0] += 0.3
    b.cam_rotation[1] += 0.1
    return a, b


def look(r, rpt, cfg, spp=SPP):
    """a new accumulator epoch under `cfg` (rpt_reset zeroes the moments record with the accumulator)"""
    r.set_config(cfg)
    r.reset(rpt.blue_noise_seeds(cfg.width, cfg.height))
    if spp:
        r.render(spp)


def begin(r, rpt, world, scene, cfg, spp=SPP):
    r.upload_scene(world(scene))
    r.set_config(cfg)
    r.set_moments(True)
    r.temporal_reset()
    look(r, rpt, cfg, spp)


def host(hipmod, r, cfg, previous, params, op=0, moments=None):
    """the host hook fed the device's accumulator, guides and moments; `previous`: what an earlier call of this function returned as "next" """
    acc, n = r.read_accum()
    if r.counts_uniform():
        mean = (acc[..., :3] / F(n)).astype(F)
    else:
        with np.errstate(all="ignore"):
            mean = np.where(acc[..., 3:] == 0, F(0.0), acc[..., :3] / acc[..., 3:]).astype(F)
    g = r.guides()
    m = r.read_moments() if moments is None else moments
    out = hipmod.denoise_temporal_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], m, cfg, previous, params, op)
    out["next"] = {"camera": cfg.copy(), "normal": g["normal"], "position": g["position"], "kind": g["kind"], "records": out["records"]}
    out["n_cur"] = m[..., 2]
    return out


def check(got, want, what):
    rgb, var, hist, rep = got
    assert same_bits(rgb, want["rgb"]), what + ": colour"
    assert same_bits(var, want["variance"]), what + ": variance"
    assert same_bits(hist, want["history"]), what + ": T"
    assert rep["pixels_with_history"] == want["pixels_with_history"] == np.count_nonzero(hist > want["n_cur"]), what
    return rep


@pytest.mark.parametrize("scene,nee", SCENES)
def test_device_equals_the_host_hook_bitwise_along_a_path(r, rpt, hipmod, world, scene, nee):
    cam_a, cam_b = views(rpt, nee)
    p = hipmod.temporal_params(iterations=2, demodulate=1, sigma_variance=SIGMA, max_history=32.0, normal_min=0.9, plane_max=2.0)
    begin(r, rpt, world, scene, cam_a)
    # A alone: no history yet, and the call is rpt_denoise_variance's
    a = host(hipmod, r, cam_a, None, p, 3)
    rep = check(r.denoise_temporal(params=p, tonemap_op=3, with_report=True), a, scene + " A")
    assert rep["history_state"] == hipmod.HISTORY_NONE and rep["pixels_with_history"] == 0 and rep["device_ms"] > 0
    plain = r.denoise_variance(params=p.filter, tonemap_op=3)
    first = r.denoise_temporal(params=p, tonemap_op=3)                                   # (a second call in A's epoch: still no history)
    assert same_bits(first[0], plain[0]) and same_bits(first[1], plain[1]) and same_bits(first[2], np.full((H, W), F(SPP)))
    # A -> B
    look(r, rpt, cam_b)
    b = host(hipmod, r, cam_b, a["next"], p, 3)
    rep = check(r.denoise_temporal(params=p, tonemap_op=3, with_report=True), b, scene + " A->B")
    assert rep["history_state"] == hipmod.HISTORY_USED and 0 < rep["pixels_with_history"] < W * H          # pixels with history and without
    assert not same_bits(r.denoise_variance(params=p.filter, tonemap_op=3)[0], b["rgb"])                    # (the history does something)
    # A -> B -> B: more samples in B's epoch blend with the SAME previous history, A's
    r.render(SPP)
    b2 = host(hipmod, r, cam_b, a["next"], p, 0)
    rep = check(r.denoise_temporal(params=p, with_report=True), b2, scene + " A->B->B")
    assert rep["pixels_with_history"] == b["pixels_with_history"] and b2["history"].max() <= 32 + 2 * SPP
    # A -> B -> A: the history is B's second call
    look(r, rpt, cam_a)
    back = host(hipmod, r, cam_a, b2["next"], p, 5)
    rep = check(r.denoise_temporal(params=p, tonemap_op=5, with_report=True), back, scene + " A->B->A")
    assert rep["history_state"] == hipmod.HISTORY_USED and 0 < rep["pixels_with_history"] < W * H


@pytest.mark.parametrize("scene,nee", SCENES)
def test_pass_counts_resolve_only_and_both_units(r, rpt, hipmod, world, scene, nee):
    """1 and 6 passes without demodulation, resolve only: every case its own A -> B (a change of `demodulate` would drop the history)"""
    cam_a, cam_b = views(rpt, nee)
    for it, dem, op in [(1, 0, 0), (6, 0, 3), (0, 1, 2)]:
        p = hipmod.temporal_params(iterations=it, demodulate=dem, sigma_variance=SIGMA, max_history=16.0, normal_min=0.8, plane_max=float("inf"))
        begin(r, rpt, world, scene, cam_a)
        a = host(hipmod, r, cam_a, None, p, op)
        check(r.denoise_temporal(params=p, tonemap_op=op, with_report=True), a, f"{scene} A, iterations {it}")
        look(r, rpt, cam_b)
        b = host(hipmod, r, cam_b, a["next"], p, op)
        rep = check(r.denoise_temporal(params=p, tonemap_op=op, with_report=True), b, f"{scene} A->B, iterations {it} demodulate {dem}")
        assert rep["history_state"] == hipmod.HISTORY_USED and rep["pixels_with_history"] > 0
        if it == 0:
            assert not same_bits(b["rgb"], r.resolve(op))


def test_per_pixel_counts_and_a_callers_moments(r, rpt, hipmod, world):
    """view B after a checkerboard rpt_render_pixels: every pixel's mean by its own count, n_cur from its own record; and a caller's moments image"""
    cam_a, cam_b = views(rpt, 0)
    p = hipmod.temporal_params(iterations=2, sigma_variance=SIGMA, max_history=32.0, normal_min=0.9, plane_max=2.0)
    begin(r, rpt, world, "DarkCornell", cam_a)
    a = host(hipmod, r, cam_a, None, p)
    r.denoise_temporal(params=p)
    look(r, rpt, cam_b)
    yy, xx = np.mgrid[0:H, 0:W]
    r.render_pixels((yy + xx) % 2 == 0, 5)
    assert not r.counts_uniform() and set(np.unique(r.read_moments()[..., 2])) == {8.0, 13.0}
    b = host(hipmod, r, cam_b, a["next"], p)
    own = r.denoise_temporal(params=p, with_report=True)
    check(own, b, "checkerboard")
    given = r.denoise_temporal(moments=r.read_moments(), params=p, with_report=True)       # (the same epoch: the same previous history)
    assert all(same_bits(x, y) for x, y in zip(given[:3], own[:3])) and given[3]["pixels_with_history"] == own[3]["pixels_with_history"]


def test_gathered_source_and_multi_equal_one_context(r, rpt, hipmod, world):
    cam_a, cam_b = views(rpt, 1)
    p = hipmod.temporal_params(iterations=3, sigma_variance=SIGMA, max_history=32.0, normal_min=0.9, plane_max=2.0)
    begin(r, rpt, world, "DarkCornell", cam_a)
    one_a = r.denoise_temporal(params=p, tonemap_op=3)
    look(r, rpt, cam_b)
    one_b = r.denoise_temporal(params=p, tonemap_op=3, with_report=True)
    assert 0 < one_b[3]["pixels_with_history"] < W * H
    # RPT_DENOISE_GATHERED on a context with a local communicator, the moments as an image
    g = hipmod.Renderer(0)
    try:
        g.upload_scene(world("DarkCornell"))
        g.set_config(cam_a)
        g.set_moments(True)
        look(g, rpt, cam_a, 0)
        g.comm_init_local()
        for cam, want in ((cam_a, one_a), (cam_b, one_b)):
            look(g, rpt, cam)
            g.gather_async()
            got = g.denoise_temporal(source=hipmod.DENOISE_GATHERED, moments=g.read_moments(), params=p, tonemap_op=3, with_report=True)
            assert all(same_bits(x, y) for x, y in zip(got[:3], want[:3]))
        assert got[3]["pixels_with_history"] == one_b[3]["pixels_with_history"] and got[3]["history_state"] == hipmod.HISTORY_USED
    finally:
        g.close()
    for ranks in (2, 3):
        m = hipmod.MultiRenderer([0] * ranks, allow_shared_device=True)
        try:
            m.upload_scene(world("DarkCornell"))
            m.set_config(cam_a)
            m.set_moments(True)
            for cam, want in ((cam_a, one_a), (cam_b, one_b)):
                m.set_config(cam)
                m.reset(rpt.blue_noise_seeds(W, H))
                m.render(SPP)
                got = m.denoise_temporal(params=p, tonemap_op=3, with_report=True)
                assert all(same_bits(x, y) for x, y in zip(got[:3], want[:3])), ranks
            assert got[3]["pixels_with_history"] == one_b[3]["pixels_with_history"]
            m.temporal_reset()
            assert m.denoise_temporal(params=p, with_report=True)[3]["history_state"] == hipmod.HISTORY_NONE
            m.render(SPP)                                                                 # still usable
            assert m.read_accum()[1] == 2 * SPP
        finally:
            m.close()


def test_what_drops_the_history(r, rpt, hipmod, world):
    """a resize, rpt_upload_scene and a change of `demodulate` drop it (history_state 2, the call is rpt_denoise_variance's); rpt_temporal_reset forgets it"""
    cam_a, cam_b = views(rpt, 0)
    p = hipmod.temporal_params(iterations=2, sigma_variance=SIGMA, demodulate=1)

    def state_after(change, params=p):
        begin(r, rpt, world, "DarkCornell", cam_a)
        r.denoise_temporal(params=p)
        cam = change() or cam_b
        look(r, rpt, cam)
        rgb, var, hist, rep = r.denoise_temporal(params=params, with_report=True)
        plain = r.denoise_variance(params=params.filter)
        assert (rep["pixels_with_history"] == 0) == (rep["history_state"] != hipmod.HISTORY_USED)
        if rep["history_state"] != hipmod.HISTORY_USED:
            assert same_bits(rgb, plain[0]) and same_bits(var, plain[1]) and (hist == SPP).all()
        after = r.denoise_temporal(params=params, with_report=True)[3]["history_state"]     # the drop is reported once
        return rep["history_state"], after

    assert state_after(lambda: None) == (hipmod.HISTORY_USED, hipmod.HISTORY_USED)
    small = views(rpt, 0, 96, 50)[1]
    assert state_after(lambda: small) == (hipmod.HISTORY_DROPPED, hipmod.HISTORY_NONE)
    assert state_after(lambda: r.upload_scene(world("DarkCornell"))) == (hipmod.HISTORY_DROPPED, hipmod.HISTORY_NONE)
    assert state_after(lambda: None, hipmod.temporal_params(iterations=2, sigma_variance=SIGMA, demodulate=0)) == (hipmod.HISTORY_DROPPED, hipmod.HISTORY_NONE)
    assert state_after(lambda: r.temporal_reset()) == (hipmod.HISTORY_NONE, hipmod.HISTORY_NONE)


def test_no_side_effects(r, rpt, hipmod, world):
    """accumulator, rng, moments, rpt_stats, the cached guides and the output of rpt_denoise and rpt_denoise_variance are the same before and after"""
    cam_a, cam_b = views(rpt, 1)
    p = hipmod.temporal_params(iterations=3, sigma_variance=SIGMA)
    begin(r, rpt, world, "VeachMIS", cam_a)
    r.denoise_temporal(params=p)
    look(r, rpt, cam_b)
    state = lambda: (r.read_accum(), r.read_rng(), r.read_moments(), {k: v for k, v in r.stats().items() if k not in ("render_ms", "kernel_ms", "kernel_launches")}, r.denoise(),
                     r.denoise_variance(params=p.filter))
    (acc0, n0), rng0, mom0, stats0, den0, var0 = state()
    mode, guides0 = r.shadow_mode(), r.guides()
    rep = r.denoise_temporal(params=p, with_report=True)[3]
    assert rep["guides_rebuilt"] == 0 and rep["device_ms"] > 0 and rep["pixels_with_history"] > 0
    r.denoise_temporal(moments=mom0 * F(2.0), params=p)                                   # a caller's image does not replace the context's record
    (acc1, n1), rng1, mom1, stats1, den1, var1 = state()
    assert n0 == n1 and same_bits(acc0, acc1) and np.array_equal(rng0, rng1) and same_bits(mom0, mom1) and stats0 == stats1 and same_bits(den0, den1)
    assert same_bits(var0[0], var1[0]) and same_bits(var0[1], var1[1])
    assert r.shadow_mode() == mode and r.moments_on() and all(same_bits(guides0[k].view(F), r.guides()[k].view(F)) for k in guides0)
    r.render(SPP)
    acc_after, n_after = r.read_accum()
    look(r, rpt, cam_b)
    r.render(SPP)
    assert r.read_accum()[1] == n_after == 2 * SPP and same_bits(r.read_accum()[0], acc_after)


def test_refusals_leave_the_context_and_its_history_usable(r, rpt, hipmod, world):
    cam_a, cam_b = views(rpt, 0)
    p = hipmod.temporal_params(iterations=2, sigma_variance=SIGMA)
    begin(r, rpt, world, "DarkCornell", cam_a)
    r.denoise_temporal(params=p)
    look(r, rpt, cam_b)
    good = r.denoise_temporal(params=p, with_report=True)
    assert good[3]["pixels_with_history"] > 0
    mom = r.read_moments()

    def refused(call, text):
        with pytest.raises(hipmod.RptError) as e:
            call()
        assert e.value.code == -1 and text in str(e.value), (text, str(e.value))
        again = r.denoise_temporal(params=p, with_report=True)                            # the next valid call succeeds, with the same bytes and history
        assert all(same_bits(x, y) for x, y in zip(again[:3], good[:3])) and again[3]["pixels_with_history"] == good[3]["pixels_with_history"], text

    refused(lambda: r.denoise_temporal(params=hipmod.temporal_params(max_history=-1.0)), "max_history")
    refused(lambda: r.denoise_temporal(params=hipmod.temporal_params(max_history=float("nan"))), "max_history")
    refused(lambda: r.denoise_temporal(params=hipmod.temporal_params(plane_max=-1.0)), "plane_max")
    refused(lambda: r.denoise_temporal(params=hipmod.temporal_params(plane_max=float("nan"))), "plane_max")
    refused(lambda: r.denoise_temporal(params=hipmod.temporal_params(normal_min=float("nan"))), "normal_min")
    refused(lambda: r.denoise_temporal(params=hipmod.temporal_params(normal_min=1.25)), "normal_min")
    refused(lambda: r.denoise_temporal(params=hipmod.temporal_params(sigma_variance=-0.5)), "sigma_variance")       # (what rpt_denoise_variance refuses)
    refused(lambda: r.denoise_temporal(params=hipmod.temporal_params(iterations=7)), "iterations")
    refused(lambda: r.denoise_temporal(params=p, tonemap_op=7), "tonemap")
    refused(lambda: r.denoise_temporal(source=hipmod.DENOISE_GATHERED, params=p), "not part of the gather")
    refused(lambda: r.denoise_temporal(source=hipmod.DENOISE_GATHERED, moments=mom, params=p), "gathered image")
    r.denoise_temporal(params=hipmod.temporal_params(iterations=2, sigma_variance=SIGMA, max_history=float("inf"), plane_max=float("inf"), normal_min=-1.0))
    L = hipmod.lib()
    assert L.rpt_denoise_temporal(r._h, 0, None, C.byref(p), 0, None, None, None, None) == -1 and b"out_rgb" in L.rpt_last_error(r._h)
    rgb = np.zeros((H, W, 3), F)
    assert L.rpt_denoise_temporal(r._h, 0, None, None, 0, rgb.ctypes.data_as(C.c_void_p), None, None, None) == 0       # every other output is nullable; params NULL
    r.set_moments(False)
    with pytest.raises(hipmod.RptError) as e:                                             # moments off with a NULL image
        r.denoise_temporal(params=p)
    assert e.value.code == -1 and "moments are off" in str(e.value)
    given = r.denoise_temporal(moments=mom, params=p)                                     # ... but a caller's image still serves
    assert all(same_bits(x, y) for x, y in zip(given, good[:3]))
    r.set_moments(True)
    r.render(SPP)
    assert r.read_accum()[1] == 2 * SPP
