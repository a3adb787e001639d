"""The moments record and the counts flag inside the gather (rpt_gather_set_moments; csrc/k_gather.h k_gather_pack, k_gather_untile2) on the device: what rank 0
holds after a gather is, bit for bit, what ONE context that rendered everything holds — the record itself, and rpt_denoise_variance / rpt_denoise_temporal
filtering by it with RPT_DENOISE_GATHERED and no moments image — on a local communicator and over 2, 3 and 5 ranks that share the device; the snapshot stays a
snapshot while the next batch renders; the per-pixel-count decision comes from the ranks' trailers; the life cycle and the refusals.

DarkCornell and VeachMIS with NEE at 100 x 70 (four tiles, three clipped; over five ranks one rank owns nothing) and 130 x 67 (six tiles), 8 spp per view."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPP = 8
F = np.float32
SIGMA = 4.0
CASES = [("DarkCornell", 100, 70), ("VeachMIS", 130, 67)]


def same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def all_same(got, want, n):
    return all(same_bits(x, y) for x, y in zip(got[:n], want[:n]))


def views(rpt, w, h):
    a = rpt.default_config(w, h, nee=1)
    b = a.copy()
    b.cam_position[0] += 0.3
    b.cam_rotation[1] += 0.1
    return a, b


def params(hipmod):
    off = hipmod.denoise_var_params(iterations=3, sigma_variance=SIGMA)
    on = hipmod.denoise_var_params(iterations=3, sigma_variance=SIGMA, **hipmod.FIREFLY_CLAMP_VARIANCE)
    tp = hipmod.temporal_params(iterations=3, sigma_variance=SIGMA, max_history=32.0, normal_min=0.9, plane_max=2.0)
    return off, on, tp


def look(r, rpt, cfg, spp=SPP):
    """a new accumulator epoch under `cfg` (Renderer and MultiRenderer alike)"""
    r.set_config(cfg)
    r.reset(rpt.blue_noise_seeds(cfg.width, cfg.height))
    if spp:
        r.render(spp)


_single = {}


@pytest.fixture(scope="module")
def single(rpt, hipmod, world):
    """what ONE context computes, once per (scene, size): after 4 and 8 samples of view A the accumulator, the record and rpt_denoise_variance (clamp off / on)
    from RPT_DENOISE_ACCUM; rpt_denoise_temporal along A -> B"""
    def compute(scene, w, h):
        if (scene, w, h) in _single:
            return _single[(scene, w, h)]
        off, on, tp = params(hipmod)
        cam_a, cam_b = views(rpt, w, h)
        r = hipmod.Renderer(0)
        try:
            r.upload_scene(world(scene))
            r.set_config(cam_a)
            r.set_moments(True)
            look(r, rpt, cam_a, SPP // 2)
            ref = {"acc4": r.read_accum()[0].copy(), "mom4": r.read_moments(), "dv4": r.denoise_variance(params=off, tonemap_op=3)}
            r.render(SPP // 2)
            ref.update(acc=r.read_accum()[0].copy(), mom=r.read_moments(), dv_off=r.denoise_variance(params=off, tonemap_op=3),
                       dv_on=r.denoise_variance(params=on, tonemap_op=3, with_report=True), dt_a=r.denoise_temporal(params=tp, tonemap_op=3))
            look(r, rpt, cam_b)
            ref.update(mom_b=r.read_moments(), dt_b=r.denoise_temporal(params=tp, tonemap_op=3, with_report=True))
            assert 0 < ref["dt_b"][3]["pixels_with_history"] < w * h
        finally:
            r.close()
        _single[(scene, w, h)] = ref
        return ref
    return compute


def local(hipmod, world, scene, cfg):
    g = hipmod.Renderer(0)
    g.upload_scene(world(scene))
    g.set_config(cfg)
    g.comm_init_local()
    return g


@pytest.mark.parametrize("scene,w,h", CASES)
def test_local_communicator(rpt, hipmod, world, single, scene, w, h):
    ref = single(scene, w, h)
    off, on, tp = params(hipmod)
    cam_a, cam_b = views(rpt, w, h)
    g = local(hipmod, world, scene, cam_a)
    try:
        assert not g.gather_moments() and not g.moments_on()
        g.gather_set_moments(True)
        assert g.gather_moments() and g.moments_on()                                      # (turned on, as render_to_noise does)
        look(g, rpt, cam_a)
        g.gather_async()
        mom = g.read_gathered_moments()
        assert same_bits(mom, g.read_moments()) and same_bits(mom, ref["mom"])
        assert same_bits(g.read_gathered()[0], ref["acc"])
        assert g.gathered_info() == {"with_moments": 1, "nonuniform": 0, "samples_min": SPP, "samples_max": SPP, "bad_trailers": 0}
        for p, want in ((off, ref["dv_off"]), (on, ref["dv_on"])):
            got = g.denoise_variance(source=hipmod.DENOISE_GATHERED, params=p, tonemap_op=3, with_report=True)
            given = g.denoise_variance(source=hipmod.DENOISE_GATHERED, moments=g.read_moments(), params=p, tonemap_op=3)
            assert all_same(got, want, 2) and all_same(given, want, 2)
        assert got[2]["pixels_clamped"] == ref["dv_on"][2]["pixels_clamped"]
        for how in ("gathered", "image"):                                                 # the two views, a reset between them (look)
            g.temporal_reset()
            for cam, want in ((cam_a, ref["dt_a"]), (cam_b, ref["dt_b"])):
                look(g, rpt, cam)
                g.gather_async()
                image = g.read_moments() if how == "image" else None
                got = g.denoise_temporal(source=hipmod.DENOISE_GATHERED, moments=image, params=tp, tonemap_op=3, with_report=True)
                assert all_same(got, want, 3), how
            assert got[3]["pixels_with_history"] == ref["dt_b"][3]["pixels_with_history"] and got[3]["history_state"] == hipmod.HISTORY_USED
        assert same_bits(g.read_gathered_moments(), ref["mom_b"])
    finally:
        g.close()


@pytest.mark.parametrize("ranks", [2, 3, 5])
@pytest.mark.parametrize("scene,w,h", CASES)
def test_several_ranks_equal_the_host_merge_and_one_context(rpt, hipmod, world, single, scene, w, h, ranks):
    ref = single(scene, w, h)
    off, on, tp = params(hipmod)
    cam_a, cam_b = views(rpt, w, h)
    m = hipmod.MultiRenderer([0] * ranks, allow_shared_device=True)
    try:
        m.upload_scene(world(scene))
        m.set_config(cam_a)
        for setting in (True, False):                                                     # off: the host-merge path (moments stay on)
            m.gather_set_moments(setting)
            assert m.gather_moments() == setting and m.moments_on()
            m.temporal_reset()
            for cam, want in ((cam_a, ref["dt_a"]), (cam_b, ref["dt_b"])):
                look(m, rpt, cam)
                if cam is cam_a:
                    assert same_bits(m.read_moments(), ref["mom"]), (setting, ranks)
                    assert all_same(m.denoise_variance(params=off, tonemap_op=3), ref["dv_off"], 2), (setting, ranks)
                    got = m.denoise_variance(params=on, tonemap_op=3, with_report=True)
                    assert all_same(got, ref["dv_on"], 2) and got[2]["pixels_clamped"] == ref["dv_on"][2]["pixels_clamped"], (setting, ranks)
                got = m.denoise_temporal(params=tp, tonemap_op=3, with_report=True)
                assert all_same(got, want, 3), (setting, ranks)
            assert got[3]["pixels_with_history"] == ref["dt_b"][3]["pixels_with_history"]
            assert same_bits(m.read_moments(), ref["mom_b"])
            info = m.gathered_info()
            assert info == {"with_moments": int(setting), "nonuniform": 0, "samples_min": SPP, "samples_max": SPP, "bad_trailers": 0}
        # switching the setting leaves no gathered image: the next reader gathers first
        m.gather_set_moments(True)
        assert same_bits(m.read_moments(), ref["mom_b"])
        assert m.read_accum()[1] == SPP
    finally:
        m.close()


@pytest.mark.parametrize("scene,w,h", CASES[:1])
def test_the_snapshot_is_a_snapshot(rpt, hipmod, world, single, scene, w, h):
    """gather after batch k, batch k + 1 enqueued behind it: the filter and the read-out see batch k; the next gather carries batch k + 1"""
    ref = single(scene, w, h)
    off, _, _ = params(hipmod)
    cam_a, _ = views(rpt, w, h)
    g = local(hipmod, world, scene, cam_a)
    try:
        g.gather_set_moments(True)
        look(g, rpt, cam_a, SPP // 2)
        g.gather_async()
        g.render_async(SPP // 2)
        got = g.denoise_variance(source=hipmod.DENOISE_GATHERED, params=off, tonemap_op=3)
        mom = g.read_gathered_moments()
        acc, n = g.read_gathered()
        assert all_same(got, ref["dv4"], 2) and same_bits(mom, ref["mom4"]) and same_bits(acc, ref["acc4"]) and n == SPP // 2
        g.gather_async()
        got = g.denoise_variance(source=hipmod.DENOISE_GATHERED, params=off, tonemap_op=3)
        assert all_same(got, ref["dv_off"], 2) and same_bits(g.read_gathered_moments(), ref["mom"]) and g.read_gathered()[1] == SPP
        assert g.gathered_info()["samples_max"] == SPP
    finally:
        g.close()


def test_per_pixel_counts_come_from_the_trailers(rpt, hipmod, world):
    """three ranks, a uniform render, then a masked pass inside one tile of rank 1: the filter divides every pixel by its own count, as the one context does"""
    w, h = 100, 70
    off, _, _ = params(hipmod)
    cam_a, _ = views(rpt, w, h)
    mask = np.zeros((h, w), np.uint8)
    mask[10:30, 70:90] = 1                                                                # inside tile 1 (x 64..99, y 0..63): rank 1 of 3
    xy = hipmod.tile_order(w, h, 1, 3)
    owned = np.zeros((h, w), bool)
    owned[xy >> 16, xy & 0xFFFF] = True
    assert owned[mask != 0].all()
    r = hipmod.Renderer(0)
    m = hipmod.MultiRenderer([0] * 3, allow_shared_device=True)
    try:
        r.upload_scene(world("DarkCornell"))
        r.set_config(cam_a)
        r.set_moments(True)
        look(r, rpt, cam_a)
        r.render_pixels(mask, 4)
        want = r.denoise_variance(params=off, tonemap_op=3)
        assert not r.counts_uniform()
        m.upload_scene(world("DarkCornell"))
        m.set_config(cam_a)
        m.gather_set_moments(True)
        look(m, rpt, cam_a)
        assert m.gathered_info()["nonuniform"] == 0
        m.render_pixels(mask, 4)
        got = m.denoise_variance(params=off, tonemap_op=3)
        assert all_same(got, want, 2)
        assert m.gathered_info() == {"with_moments": 1, "nonuniform": 1, "samples_min": SPP, "samples_max": SPP, "bad_trailers": 0}
        assert same_bits(m.read_moments(), r.read_moments())
    finally:
        m.close()
        r.close()


def test_life_cycle_and_refusals(rpt, hipmod, world, single):
    scene, w, h = CASES[0]
    ref = single(scene, w, h)
    off, _, tp = params(hipmod)
    cam_a, _ = views(rpt, w, h)
    L = hipmod.lib()
    plain = hipmod.Renderer(0)
    g = local(hipmod, world, scene, cam_a)
    m = hipmod.MultiRenderer([0] * 2, allow_shared_device=True)
    try:
        # without a communicator
        plain.upload_scene(world(scene))
        look(plain, rpt, cam_a, 0)
        with pytest.raises(hipmod.RptError) as e:
            plain.gather_set_moments(True)
        assert e.value.code == -1 and "no communicator" in str(e.value)
        assert not plain.moments_on()
        plain.render(SPP)
        assert same_bits(plain.read_accum()[0], ref["acc"])

        g.gather_set_moments(True)
        look(g, rpt, cam_a, 0)

        def refused(call, text, usable=True):
            with pytest.raises(hipmod.RptError) as e:
                call()
            assert e.value.code == -1 and text in str(e.value), (text, str(e.value))
            if usable:                                                                    # the next valid call succeeds, with the same bytes
                again = g.denoise_variance(source=hipmod.DENOISE_GATHERED, params=off, tonemap_op=3)
                assert all_same(again, ref["dv_off"], 2), text

        # before a gather has carried moments
        refused(lambda: g.denoise_variance(source=hipmod.DENOISE_GATHERED, params=off), "no gather has carried the moments", usable=False)
        refused(lambda: g.denoise_temporal(source=hipmod.DENOISE_GATHERED, params=tp), "no gather has carried the moments", usable=False)
        refused(g.read_gathered_moments, "no gather has carried the moments", usable=False)
        refused(g.gathered_moments_device_ptr, "no gather has carried the moments", usable=False)
        refused(g.gathered_info, "after the first gather", usable=False)
        g.render(SPP)
        g.gather_async()
        assert all_same(g.denoise_variance(source=hipmod.DENOISE_GATHERED, params=off, tonemap_op=3), ref["dv_off"], 2)
        assert g.gathered_moments_device_ptr()
        # the record cannot be turned off under the gather
        refused(lambda: g.set_moments(False), "rpt_gather_set_moments(ctx, 0)")
        assert g.moments_on() and g.gather_moments()
        # null pointers
        assert L.rpt_gather_set_moments(None, 1) == -1 and L.rpt_gather_moments(g._h, None) == -1 and L.rpt_read_gathered_moments(g._h, None) == -1
        assert L.rpt_gathered_moments_device_ptr(g._h, None) == -1 and L.rpt_gathered_info_get(g._h, None) == -1 and L.rpt_multi_gather_set_moments(None, 1) == -1
        assert all_same(g.denoise_variance(source=hipmod.DENOISE_GATHERED, params=off, tonemap_op=3), ref["dv_off"], 2)
        # after a resize, until the next gather
        g.set_config(rpt.default_config(w + 8, h, nee=1))
        refused(lambda: g.denoise_variance(source=hipmod.DENOISE_GATHERED, params=off), "resized", usable=False)
        refused(g.read_gathered_moments, "resized", usable=False)
        look(g, rpt, cam_a)
        g.gather_async()
        assert all_same(g.denoise_variance(source=hipmod.DENOISE_GATHERED, params=off, tonemap_op=3), ref["dv_off"], 2)
        assert same_bits(g.read_gathered_moments(), ref["mom"])
        # reset zeroes the record, and the next gather carries the zeroed one
        g.reset(rpt.blue_noise_seeds(w, h))
        assert same_bits(g.read_gathered_moments(), ref["mom"])                           # (still the last gather's)
        g.gather_async()
        assert not g.read_gathered_moments().view(np.uint32).any() and g.gathered_info()["samples_max"] == 0
        g.render(SPP)
        g.gather_async()
        assert same_bits(g.read_gathered_moments(), ref["mom"])

        # a rank other than 0
        m.upload_scene(world(scene))
        m.set_config(cam_a)
        m.gather_set_moments(True)
        look(m, rpt, cam_a)
        one = m.rank_view(1)
        for call in (one.read_gathered_moments, one.gathered_moments_device_ptr, one.gathered_info,
                     lambda: one.denoise_variance(source=hipmod.DENOISE_GATHERED, params=off)):
            with pytest.raises(hipmod.RptError) as e:
                call()
            assert e.value.code == -1 and "rank 0" in str(e.value)
        with pytest.raises(hipmod.RptError) as e:
            m.set_moments(False)
        assert e.value.code == -1 and "rpt_gather_set_moments(ctx, 0)" in str(e.value) and m.moments_on()
        assert all_same(m.denoise_variance(params=off, tonemap_op=3), ref["dv_off"], 2)

        # the setting off: the plain gather's bits and today's refusals
        g.gather_set_moments(False)
        assert not g.gather_moments() and g.moments_on()
        with pytest.raises(hipmod.RptError) as e:
            g.read_gathered()
        assert "after the first gather" in str(e.value)
        g.gather_async()
        assert same_bits(g.read_gathered()[0], ref["acc"])
        assert g.gathered_info() == {"with_moments": 0, "nonuniform": 0, "samples_min": SPP, "samples_max": SPP, "bad_trailers": 0}
        for call, text in ((lambda: g.denoise_variance(source=hipmod.DENOISE_GATHERED, params=off), "not part of the gather"),
                           (lambda: g.denoise_temporal(source=hipmod.DENOISE_GATHERED, params=tp), "not part of the gather"),
                           (g.read_gathered_moments, "does not carry the moments"), (g.gathered_moments_device_ptr, "does not carry the moments")):
            with pytest.raises(hipmod.RptError) as e:
                call()
            assert e.value.code == -1 and text in str(e.value)
        given = g.denoise_variance(source=hipmod.DENOISE_GATHERED, moments=g.read_moments(), params=off, tonemap_op=3)
        assert all_same(given, ref["dv_off"], 2)
        g.set_moments(False)                                                              # allowed again
        assert not g.moments_on()
    finally:
        m.close()
        g.close()
        plain.close()
