"""The thin-lens camera on the device (rpt_set_camera_lens; csrc/rpt_lens.hip k_generate_lens, k_lens_complete, k_lens_complete_moments, k_dn_camera_rays_lens):
the device's rays against the host build of csrc/k_lens.h, accumulators, rng and counters word for word against the restatement tests/lens_oracle — from LDS
(aperture 0: the FIRST walk over prepared slots; an aperture: the plain walk) and from global memory, every NEE mode, every route into the pipeline — the
default record against a context that never set one, the guides and the filters under a lens, and every refusal.  80 x 72 (a whole tile, a 16-pixel and an
8-pixel remainder), 8 spp unless stated.  Material models under a lens: tests/test_gpu_models_lens.py."""
import ctypes as C
import os

import numpy as np
import pytest

import denoise_ref
import lens_ref
import moments_ref
from lens_ref import F, LENSES

pytestmark = pytest.mark.gpu

W, H, SPP = 80, 72, 8
IMAGE_LENSES = ["fov", "both"]          # aperture 0 and an aperture: the two dispatches of iteration 0


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def counters_match(gs, st):
    got = (gs["extension_rays"], gs["shadow_rays"], gs["sky_evals"], gs["shadow_rays_elided"])
    want = (st.extension_rays, st.shadow_rays, st.sky_evals, st.shadow_rays_zero_term)
    assert got == want, (got, want)


class context:
    """a Renderer of its own (the developer knobs are read by rpt_create) with the given environment"""

    def __init__(self, hipmod, env=None, in_flight=None, partition=None):
        old = {k: os.environ.get(k) for k in (env or {})}
        os.environ.update(env or {})
        try:
            self.r = hipmod.Renderer(0) if partition is None else hipmod.Renderer(0, *partition)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        if in_flight is not None:
            self.r.set_samples_in_flight(in_flight)

    def __enter__(self):
        return self.r

    def __exit__(self, *exc):
        self.r.close()


def prepare(r, rpt, world, which, nee, lens_name, **more):
    w, skybox, _ = lens_ref.scene_and_view(world, which)
    r.upload_scene(w, skybox_f32=skybox)
    r.set_config(lens_ref.config(world, which, nee, W, H, **more))
    r.set_camera_lens(lens_ref.lens(lens_name))
    r.reset(rpt.blue_noise_seeds(W, H))


def check_against(r, ref, spp=SPP, counters=True):
    acc, rng, st = ref
    got, n = r.read_accum()
    assert n == spp and same_words(got, acc), f"{int((got.view(np.uint32) != acc.view(np.uint32)).any(-1).sum())} pixels differ"
    assert np.array_equal(r.read_rng().reshape(-1), np.asarray(rng).reshape(-1))
    if counters:
        counters_match(r.stats(), st)


def reference(oracle, world, which, nee, lens_name, spp=SPP):
    return lens_ref.reference(oracle, world, which, nee, lens_name, W, H, spp)


@pytest.mark.parametrize("name", sorted(LENSES))
def test_device_rays_are_the_host_hook_bit_for_bit(renderer, hipmod, rpt, world, name):
    cfg = rpt.default_config(333, 187, cam_position=(0.3, 1.1, -2.4, 0.0), cam_rotation=(0.21, -0.47, 0.0, 0.0))
    renderer.upload_scene(world("DarkCornell"))
    renderer.set_config(cfg)
    renderer.set_camera_lens(lens_ref.lens(name))
    try:
        xy, keys = lens_ref.pairs(333, 187)
        o, d = renderer.debug_lens_rays(xy, keys)
        want_o, want_d = hipmod.lens_rays_host(cfg, lens_ref.lens(name), xy, keys)
        assert same_words(o, want_o) and same_words(d, want_d)
    finally:
        renderer.set_camera_lens(None)


@pytest.mark.parametrize("lens_name", IMAGE_LENSES)
@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("which,env", [("DarkCornell", {}), ("DarkCornell", {"RPT_NO_LDS_SCENE": "1"}), ("textured", {})])
def test_words_and_counters_are_the_restatements(hipmod, rpt, oracle, world, which, env, nee, lens_name, monkeypatch):
    """DarkCornell lives in LDS — aperture 0 takes the FIRST walk, an aperture the plain one —, with RPT_NO_LDS_SCENE=1 it is walked from global memory"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)                         # rpt_upload_scene reads RPT_NO_LDS_SCENE AGAIN: in the environment until the scene is up
    with context(hipmod, env) as r:
        prepare(r, rpt, world, which, nee, lens_name)
        if which == "DarkCornell":
            assert (r.last_bounce_order()["mode"] == 0) == bool(env)      # (the LAST walk needs the LDS image: off where the scene is walked from global memory)
        r.render(SPP)                                    # a batch of known length: no slot takes a second sample
        check_against(r, reference(oracle, world, which, nee, lens_name))
        assert r.stats()["kernel_launches"]["generate"] == 1


@pytest.mark.parametrize("lens_name", IMAGE_LENSES)
@pytest.mark.parametrize("q_shift", [None, "2"])
def test_slots_that_take_several_samples(hipmod, rpt, oracle, world, lens_name, q_shift):
    """20 spp with 4 samples in flight, polled: the lens completion kernels restart the finished slots (slot k takes k, k + 4, ...), at q_shift 0 from the
    registers and at RPT_SLOT_Q_SHIFT=2 through complete_restart_rows"""
    with context(hipmod, {} if q_shift is None else {"RPT_SLOT_Q_SHIFT": q_shift}, in_flight=4) as r:
        prepare(r, rpt, world, "DarkCornell", 1, lens_name)
        r.render(20)
        check_against(r, reference(oracle, world, "DarkCornell", 1, lens_name, 20), 20)


@pytest.mark.parametrize("lens_name", IMAGE_LENSES)
def test_two_batches_and_an_asynchronous_one(renderer, rpt, oracle, world, lens_name):
    try:
        prepare(renderer, rpt, world, "DarkCornell", 1, lens_name)
        renderer.render(3)
        renderer.render(5)
        check_against(renderer, reference(oracle, world, "DarkCornell", 1, lens_name))
        renderer.reset(rpt.blue_noise_seeds(W, H))
        renderer.render_async(SPP)
        renderer.wait()
        check_against(renderer, reference(oracle, world, "DarkCornell", 1, lens_name))
    finally:
        renderer.set_camera_lens(None)


@pytest.mark.parametrize("lens_name", IMAGE_LENSES)
def test_masked_pass_over_a_checkerboard(hipmod, rpt, oracle, world, lens_name):
    acc, rng, _ = reference(oracle, world, "DarkCornell", 1, lens_name)
    y, x = np.mgrid[0:H, 0:W]
    mask = (x + y) % 2 == 0
    with context(hipmod) as r:
        prepare(r, rpt, world, "DarkCornell", 1, lens_name)
        r.render_pixels(mask, SPP)
        got, _ = r.read_accum()
        assert same_words(got[mask], acc[mask]) and not got[~mask].any()
        assert np.array_equal(r.read_rng().reshape(H, W)[mask], np.asarray(rng).reshape(H, W)[mask])


@pytest.mark.parametrize("lens_name", IMAGE_LENSES)
@pytest.mark.parametrize("in_flight,spp", [(None, SPP), (2, 5)])
def test_moments_on(hipmod, rpt, oracle, world, lens_name, in_flight, spp):
    """k_lens_complete_moments, in one completion of a batch of known length and restarting slots (5 samples through 2 slots): the image is the restatement's,
    the record is tests/moments_ref.py over the restatement's per-sample radiances"""
    samples = lens_ref.per_sample_radiances(oracle, world, "DarkCornell", 1, lens_name, W, H, SPP)
    want = np.zeros((H, W, 4), F)
    for k in range(spp):
        moments_ref.add_sample(want, samples[k])
    with context(hipmod, in_flight=in_flight) as r:
        r.set_moments(True)
        prepare(r, rpt, world, "DarkCornell", 1, lens_name)
        r.render(spp)
        if spp == SPP:
            check_against(r, reference(oracle, world, "DarkCornell", 1, lens_name))
        else:
            acc = np.zeros((H, W, 4), F)
            for k in range(spp):
                acc[..., :3] = acc[..., :3] + samples[k]
                acc[..., 3] = acc[..., 3] + F(1)
            assert same_words(r.read_accum()[0], acc)
        assert same_words(r.read_moments(), want)


def test_rank_one_of_three(hipmod, rpt, oracle, world):
    acc, _, _ = reference(oracle, world, "DarkCornell", 1, "both")
    xy = hipmod.tile_order(W, H, 1, 3)
    own = np.zeros((H, W), bool)
    own[xy >> 16, xy & 0xFFFF] = True
    with context(hipmod, partition=(1, 3)) as r:
        prepare(r, rpt, world, "DarkCornell", 1, "both")
        r.render(SPP)
        got, _ = r.read_accum()
        assert own.any() and same_words(got[own], acc[own]) and not got[~own].any()


def test_three_ranks_on_one_device(hipmod, rpt, oracle, world):
    """rpt_multi_set_camera_lens: the gathered image of three ranks is the one-context image (the restatement's), the counters sum to its"""
    acc, _, st = reference(oracle, world, "DarkCornell", 1, "both")
    m = hipmod.MultiRenderer([0, 0, 0], allow_shared_device=True)
    try:
        m.upload_scene(world("DarkCornell"))
        m.set_config(lens_ref.config(world, "DarkCornell", 1, W, H))
        m.set_camera_lens(lens_ref.lens("both"))
        m.reset(rpt.blue_noise_seeds(W, H))
        m.render(SPP)
        got, n = m.read_accum()
        assert n == SPP and same_words(got, acc)
        counters_match(m.stats(), st)
    finally:
        m.close()


@pytest.mark.parametrize("nee", [0, 1])
def test_the_default_record_set_explicitly_changes_nothing(hipmod, rpt, world, nee):
    """images, rng, counters and kernel launches of a context that set {1, 0, 1, 0} — and an inactive record with another focus, and NULL — equal those of a
    context that never called the setter: a known-length batch, a polled call and an asynchronous one"""
    def run(set_lens):
        with context(hipmod) as r:
            r.upload_scene(world("DarkCornell"))
            r.set_config(lens_ref.config(world, "DarkCornell", nee, W, H))
            if set_lens is not False:
                r.set_camera_lens(set_lens)
            r.reset(rpt.blue_noise_seeds(W, H))
            r.render(SPP)
            r.set_samples_in_flight(4)
            r.reset(rpt.blue_noise_seeds(W, H), accum_init=r.read_accum()[0], samples_init=SPP)
            r.render(9)
            r.render_async(3)
            r.wait()
            st = r.stats()
            return r.read_accum()[0].copy(), r.read_rng().copy(), {k: st[k] for k in ("samples", "extension_rays", "shadow_rays", "shadow_rays_elided", "sky_evals", "iterations")}, st["kernel_launches"]
    base = run(False)
    for record in (lens_ref.lens((1.0, 0.0, 1.0)), lens_ref.lens((1.0, 0.0, 42.0)), None):
        acc, rng, counters, launches = run(record)
        assert same_words(acc, base[0]) and np.array_equal(rng, base[1]) and counters == base[2] and launches == base[3]


def test_one_slot_per_pixel_is_refused_by_name(hipmod, rpt, oracle, world):
    with context(hipmod, in_flight=1) as r:
        prepare(r, rpt, world, "DarkCornell", 1, "fov")
        with pytest.raises(hipmod.RptError) as e:
            r.render(SPP)
        assert e.value.code == -1 and "camera lens" in str(e.value) and "rpt_set_samples_in_flight" in str(e.value)
        r.set_camera_lens(None)                          # the way out the message names
        r.render(SPP)
        assert r.read_accum()[1] == SPP
    with context(hipmod, in_flight=2) as r:              # a one-sample call uses slot 0 of 2 and passes through the completion kernel
        prepare(r, rpt, world, "DarkCornell", 1, "fov")
        r.render(1)
        check_against(r, reference(oracle, world, "DarkCornell", 1, "fov", 1), 1)


@pytest.mark.parametrize("lens_name", ["fov", "both", "aperture"])
def test_guides_under_a_lens_are_the_numpy_restatement(renderer, rpt, oracle, world, monkeypatch, lens_name):
    """rpt_read_guides == tests/denoise_ref.py's guides fed the lens-centre rays, every plane bit for bit; the aperture does not enter ("aperture": the
    reference camera's guides)"""
    cfg = rpt.default_config(W, H, cam_rotation=(-0.3, 0.1, 0.0, 0.0))      # pitched up: the lamp is in view under every one of the three lenses
    wld = world("DarkCornell")
    try:
        renderer.upload_scene(wld)
        renderer.set_config(cfg)
        renderer.set_camera_lens(lens_ref.lens(lens_name))
        got = renderer.guides()
    finally:
        renderer.set_camera_lens(None)
    monkeypatch.setattr(denoise_ref, "camera_rays", lambda c, orc: lens_ref.centre_rays(c, LENSES[lens_name][0], orc))
    want = denoise_ref.guides(wld, cfg, oracle)
    assert len(np.unique(want["kind"])) >= 2
    for plane in ("kind", "depth", "albedo", "normal", "position"):
        g, w = np.ascontiguousarray(got[plane]), np.ascontiguousarray(want[plane])
        differing = int((g.view(np.uint32) != w.view(np.uint32)).sum())
        print(f"{lens_name} {plane}: {differing} words differ" + (f", max abs {np.abs(g.astype(np.float64) - w.astype(np.float64)).max():.3e}" if plane != "kind" else ""))
    for plane in ("kind", "depth", "albedo", "normal", "position"):
        assert np.array_equal(np.ascontiguousarray(got[plane]).view(np.uint32), np.ascontiguousarray(want[plane]).view(np.uint32)), plane
    if lens_name == "aperture":
        renderer.set_config(cfg)
        plain = renderer.guides()
        assert all(np.array_equal(np.ascontiguousarray(plain[k]).view(np.uint32), np.ascontiguousarray(got[k]).view(np.uint32)) for k in plain)


def same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.mark.parametrize("lens_name", ["fov", "both"])
def test_filters_under_a_lens_equal_their_host_builds(hipmod, rpt, world, lens_name):
    """rpt_denoise and rpt_denoise_variance: device == host build bit for bit, the host builds handed sigma_plane * tan_half_fov (the one route the field of
    view takes into the plane term, 2 tan_half_fov / W); a lens change rebuilds the guides; rpt_denoise_temporal under a field of view is refused by name"""
    tan_half = F(LENSES[lens_name][0])
    with context(hipmod) as r:
        r.set_moments(True)
        prepare(r, rpt, world, "DarkCornell", 1, lens_name)
        r.render(SPP)
        acc, n = r.read_accum()
        mean = (acc[..., :3] / F(n)).astype(F)
        g = r.guides()
        for it, sp in [(2, 1.0), (3, 0.37)]:
            dev, rep = r.denoise(params=hipmod.denoise_params(iterations=it, sigma_plane=sp), with_report=True)
            host = hipmod.denoise_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], hipmod.denoise_params(iterations=it, sigma_plane=float(F(sp) * tan_half)), 0)
            assert same_bits(dev, host), (it, sp)
            unscaled = hipmod.denoise_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], hipmod.denoise_params(iterations=it, sigma_plane=sp), 0)
            assert not same_bits(dev, unscaled)          # (the factor is there)
            vdev = r.denoise_variance(params=hipmod.denoise_var_params(iterations=it, sigma_plane=sp, sigma_variance=4.0))
            vhost = hipmod.denoise_variance_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], r.read_moments(),
                                                 hipmod.denoise_var_params(iterations=it, sigma_plane=float(F(sp) * tan_half), sigma_variance=4.0), 0)
            assert same_bits(vdev[0], vhost[0]) and same_bits(vdev[1], vhost[1]), (it, sp)
        assert r.denoise(with_report=True)[1]["guides_rebuilt"] == 0
        with pytest.raises(hipmod.RptError) as e:
            r.denoise_temporal()
        assert e.value.code == -1 and "rpt_denoise_temporal" in str(e.value) and "field of view" in str(e.value)
        r.set_camera_lens(lens_ref.lens("aperture"))     # an aperture alone: the projection is the reference camera's
        assert r.denoise(with_report=True)[1]["guides_rebuilt"] == 1
        r.denoise_temporal()
        r.set_camera_lens(lens_ref.lens("aperture"))     # the same record again: the guides stay
        assert r.denoise(with_report=True)[1]["guides_rebuilt"] == 0


def test_refusals_leave_the_lens_as_it_was(hipmod, rpt, world):
    with context(hipmod) as r:
        prepare(r, rpt, world, "DarkCornell", 1, "both")
        kept = LENSES["both"]

        def refused(record, reason, code=-1, reserved=0):
            rec = lens_ref.lens(record)
            rec.reserved = reserved
            with pytest.raises(hipmod.RptError) as e:
                r.set_camera_lens(rec)
            assert e.value.code == code and reason in str(e.value), (record, str(e.value))
            now = r.camera_lens()
            assert (now.tan_half_fov, now.aperture_radius, now.focus_distance, now.reserved) == tuple(float(F(v)) for v in kept) + (0,)

        for t in (0.0, -1.0, np.inf, np.nan):
            refused((t, 0.0, 1.0), "tan_half_fov")
        for a in (-0.1, np.inf, np.nan):
            refused((1.0, a, 1.0), "aperture_radius")
        for f in (0.0, -2.0, np.inf, np.nan):
            refused((1.0, 0.1, f), "focus_distance")
        refused((1.0, 0.0, 1.0), "reserved", reserved=7)
        r.set_camera_lens(lens_ref.lens((2.0, 0.0, np.nan)))       # the focus is read only with an aperture
        kept = (2.0, 0.0, np.nan)
        now = r.camera_lens()
        assert now.tan_half_fov == 2.0 and now.aperture_radius == 0.0 and np.isnan(now.focus_distance)

        # the dimension budget: MIS with 4 bounces needs 30 (2 + 4 * 7), with roulette from bounce 3 on 31 — entry 31 is the lens sample's
        d30, d31 = dict(max_bounces=4, min_bounces=3), dict(max_bounces=4, min_bounces=2)
        r.set_camera_lens(lens_ref.lens("both"))
        kept = LENSES["both"]
        r.set_config(lens_ref.config(world, "DarkCornell", 1, W, H, **d30))             # 30 passes with an aperture
        with pytest.raises(hipmod.RptError) as e:                                        # the configuration comes second
            r.set_config(lens_ref.config(world, "DarkCornell", 1, W, H, **d31))
        assert e.value.code == -4 and "31" in str(e.value) and "rpt_set_config" in str(e.value)
        r.reset(rpt.blue_noise_seeds(W, H))
        r.render(2)                                                                      # ... and the context renders on with the configuration it had
        r.set_camera_lens(lens_ref.lens("fov"))                                          # no aperture: 31 dimensions are the configuration's to use
        kept = LENSES["fov"]
        r.set_config(lens_ref.config(world, "DarkCornell", 1, W, H, **d31))
        refused(LENSES["both"], "31", code=-4)                                           # the lens comes second
        refused(LENSES["aperture"], "rpt_set_camera_lens", code=-4)
        r.set_config(rpt.default_config(W, H, nee=1))                                    # the default MIS configuration needs 30
        r.set_camera_lens(lens_ref.lens("both"))
        kept = LENSES["both"]

        # while an asynchronous batch is pending
        r.reset(rpt.blue_noise_seeds(W, H))
        r.render_async(SPP)
        refused(LENSES["fov"], "pending")
        r.wait()
        r.set_camera_lens(lens_ref.lens("fov"))
