"""Punctual lights on the device (rpt_set_punctual_lights; csrc/rpt_punctual.hip k_shade_punctual): accumulators, rng and counters word for word against the
restatement tests/lights_oracle, in both NEE modes, both shade layouts and both slot layouts, through every call shape and route into the pipeline; nee 0 and
a context without lights against the run without this feature, byte for byte and launch for launch; the forced variant; life cycle and refusals.  80 x 72 (a
whole tile, a 16-pixel and an 8-pixel remainder) and 37 x 23 (partial 8 x 8 blocks), 8 spp."""
import os

import numpy as np
import pytest

import lens_ref
import lights_ref
import model_scenes
import moments_ref
import scenes
import volume_ref
from lights_ref import SHARE, same_bits_or_both_nan

pytestmark = pytest.mark.gpu

W, H, SPP = 80, 72, 8
F = np.float32
SHADE, SHADE_MODELS, SHADE_VOLUMES, SHADE_PUNCTUAL = 0, 1, 2, 3              # rpt_debug_last_shade_variant


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def reference(oracle, name, nee, size=(W, H), spp=SPP, lens=None, vols=None, lts="scene", shadow_mode=0):
    return lights_ref.reference(oracle, name, nee, size[0], size[1], spp, lens=lens, vols=vols, lts=lts, shadow_mode=shadow_mode,
                                **model_scenes.lens_overrides(nee, lens))


def counters_match(gs, st):
    got = (gs["extension_rays"], gs["shadow_rays"], gs["sky_evals"], gs["shadow_rays_elided"])
    want = (st.extension_rays, st.shadow_rays, st.sky_evals, st.shadow_rays_zero_term)
    assert got == want, (got, want)


_renderers = {}


@pytest.fixture(scope="module")
def variants(hipmod):
    """one context per (RPT_SHADE_COMPACT, RPT_SLOT_Q_SHIFT): both are read by rpt_create"""
    def get(compact=0, q_shift=0):
        key = (compact, q_shift)
        if key not in _renderers:
            old = {k: os.environ.get(k) for k in ("RPT_SHADE_COMPACT", "RPT_SLOT_Q_SHIFT")}
            os.environ["RPT_SHADE_COMPACT"], os.environ["RPT_SLOT_Q_SHIFT"] = str(compact), str(q_shift)
            try:
                _renderers[key] = hipmod.Renderer(0)
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        return _renderers[key]
    yield get
    for r in _renderers.values():
        r.close()
    _renderers.clear()


def prepare(r, rpt, name, nee, size=(W, H), lens=None, vols=None, lts="scene", share=SHARE):
    """scene, records, lights, configuration, lens, reset (the lens is taken off first: a context that holds an aperture refuses a 31-dimension configuration)"""
    w, rec, skybox, _ = model_scenes.scene(name)
    rec_v = volume_ref.volumes(name) if isinstance(vols, str) else vols
    rec_l = lights_ref.lights(name) if isinstance(lts, str) else lts
    r.set_camera_lens(None)
    r.debug_force_punctual_kernels(False)
    r.set_shadow_mode(0)
    r.upload_scene(w, skybox_f32=skybox)                      # (clears the records and the lights)
    r.set_material_models(rec)
    if rec_v is not None:
        r.set_material_volumes(rec_v)
    r.set_punctual_lights(rec_l, share)
    r.set_config(model_scenes.config(name, nee, size[0], size[1], **model_scenes.lens_overrides(nee, lens)))
    r.set_camera_lens(lens_ref.lens(lens))
    r.reset(rpt.blue_noise_seeds(*size))


def check_against(r, ref, spp=SPP, counters=True):
    acc, rng, st = ref
    got, n = r.read_accum()
    assert n == spp and same_words(got, acc), f"{int((got.view(np.uint32) != acc.view(np.uint32)).any(-1).sum())} pixels differ"
    assert np.array_equal(r.read_rng().reshape(-1), np.asarray(rng).reshape(-1))
    if counters:
        counters_match(r.stats(), st)


def launches(r):
    return dict(r.stats()["kernel_launches"])


def test_the_device_hook_is_the_host_hook(variants, hipmod):
    for lts, q, hits, l1 in lights_ref.sample_inputs():
        got, want = variants().debug_punctual_sample(lts, q, hits, l1), hipmod.debug_punctual_sample_host(lts, q, hits, l1)
        assert np.array_equal(got[0], want[0])
        assert all(same_bits_or_both_nan(g, w_) for g, w_ in zip(got[1:], want[1:]))


@pytest.mark.parametrize("q_shift", [0, 5])
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("nee", [1, 2])
@pytest.mark.parametrize("name", ["room", "small_room", "open", "textured"])
def test_words_and_counters_are_the_restatements(variants, rpt, oracle, name, nee, compact, q_shift):
    """small_room and textured live in LDS; open has no emissive triangle (q = 1: the draws are now made), the others have (mesh and punctual picks both occur)"""
    r = variants(compact, q_shift)
    prepare(r, rpt, name, nee)
    r.render(SPP)                                        # a batch of known length: no slot takes a second sample
    assert r.debug_last_shade_variant() == SHADE_PUNCTUAL
    ref = reference(oracle, name, nee)
    st = ref[2]
    assert st.punctual_picks > 0
    if name == "open":
        assert st.punctual_picks == st.shadow_rays and r.punctual_lights()[1] == 1.0
    else:
        assert st.shadow_rays - st.punctual_picks > 0 and r.punctual_lights()[1] == F(SHARE)
    check_against(r, ref)


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("nee", [1, 2])
@pytest.mark.parametrize("name", ["room", "textured"])
def test_an_image_of_partial_blocks(variants, rpt, oracle, name, nee, compact):
    r = variants(compact, 0)
    prepare(r, rpt, name, nee, size=(37, 23))
    r.render(SPP)
    check_against(r, reference(oracle, name, nee, size=(37, 23)))


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_two_batches_and_an_asynchronous_one(variants, rpt, oracle, name):
    r = variants()
    prepare(r, rpt, name, 2)
    r.render(3)
    r.render(5)
    check_against(r, reference(oracle, name, 2))
    r.reset(rpt.blue_noise_seeds(W, H))
    r.render_async(SPP)
    r.wait()
    check_against(r, reference(oracle, name, 2))


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("in_flight", [2, 1])
def test_the_polled_route_slots_that_take_several_samples(hipmod, rpt, oracle, compact, in_flight, monkeypatch):
    monkeypatch.setenv("RPT_SHADE_COMPACT", str(compact))
    r = hipmod.Renderer(0)
    try:
        r.set_samples_in_flight(in_flight)
        prepare(r, rpt, "room", 2)
        r.render(SPP)
        check_against(r, reference(oracle, "room", 2))
    finally:
        r.close()


def test_masked_pass_over_a_checkerboard(hipmod, rpt, oracle):
    acc, rng, _ = reference(oracle, "room", 1)
    y, x = np.mgrid[0:H, 0:W]
    mask = (x + y) % 2 == 0
    r = hipmod.Renderer(0)
    try:
        prepare(r, rpt, "room", 1)
        r.render_pixels(mask, SPP)
        got, _ = r.read_accum()
        assert same_words(got[mask], acc[mask]) and not got[~mask].any()
        assert np.array_equal(r.read_rng().reshape(H, W)[mask], np.asarray(rng).reshape(H, W)[mask])
    finally:
        r.close()


def test_moments_on(hipmod, rpt, oracle):
    """the record equals tests/moments_ref.py over the restatement's per-sample radiances"""
    samples, picks, _ = lights_ref.per_sample(oracle, "room", 1, W, H, SPP)
    assert picks.any()
    want, acc = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    for k in range(SPP):
        moments_ref.add_sample(want, samples[k])
        acc[..., :3] = acc[..., :3] + samples[k]
        acc[..., 3] = acc[..., 3] + F(1)
    r = hipmod.Renderer(0)
    try:
        r.set_moments(True)
        prepare(r, rpt, "room", 1)
        r.render(SPP)
        check_against(r, reference(oracle, "room", 1))
        assert same_words(r.read_accum()[0], acc)
        assert same_words(r.read_moments(), want)
    finally:
        r.close()


@pytest.mark.parametrize("nee", [1, 2])
@pytest.mark.parametrize("name", ["room", "small_room"])
def test_a_lens_with_an_aperture(variants, rpt, oracle, name, nee):
    """"both" of tests/lens_ref.py, with model_scenes.APERTURE_OVERRIDES: k_generate_lens scatters the origins"""
    r = variants()
    try:
        prepare(r, rpt, name, nee, lens="both")
        r.render(SPP)
        check_against(r, reference(oracle, name, nee, lens="both"))
    finally:
        r.set_camera_lens(None)


@pytest.mark.parametrize("nee", [1, 2])
def test_glass_and_lambertian_records_with_volumes(variants, rpt, oracle, nee):
    """the room's Glass sphere and pane absorb (rpt_set_material_volumes) while the lights are set: one variant serves both"""
    r = variants()
    prepare(r, rpt, "room", nee, vols="scene")
    r.render(SPP)
    assert r.debug_last_shade_variant() == SHADE_PUNCTUAL
    ref = reference(oracle, "room", nee, vols="scene")
    assert ref[2].segments_absorbed > 0 and ref[2].punctual_picks > 0
    check_against(r, ref)


@pytest.mark.parametrize("nee", [1, 2])
@pytest.mark.parametrize("name", ["room", "small_room", "open", "textured"])
def test_segment_bounded_shadow_walks(variants, hipmod, rpt, oracle, name, nee, capsys):
    """rpt_set_shadow_mode's segment mode against the restatement's own mode for it (a child box is entered only if also tmin <= max_t, for mesh and punctual
    shadow rays alike: tests/lights_oracle shadow_ray_hits, held to tools/anyhit_order_sim.cpp ray by ray in tests/test_punctual_lights.py): accumulators, rng
    and counters word for word; then the exact mode on the same context, against the exact restatement: the segment batch left nothing behind"""
    r = variants()
    prepare(r, rpt, name, nee)
    try:
        r.set_shadow_mode(hipmod.SHADOW_SEGMENT)
        r.render(SPP)
        assert r.debug_last_shade_variant() == SHADE_PUNCTUAL
        segment, exact = reference(oracle, name, nee, shadow_mode=1), reference(oracle, name, nee)
        with capsys.disabled():
            print(f"\n{name} nee {nee}: {int((segment[0].view(np.uint32) != exact[0].view(np.uint32)).any(-1).sum())} pixels differ between the two modes' restatements", end="")
        check_against(r, segment)
        r.set_shadow_mode(hipmod.SHADOW_EXACT)
        r.reset(rpt.blue_noise_seeds(W, H))
        r.render(SPP)
        check_against(r, exact)
    finally:
        r.set_shadow_mode(hipmod.SHADOW_EXACT)


def test_rank_one_of_three(hipmod, rpt, oracle):
    acc, _, _ = reference(oracle, "room", 1)
    xy = hipmod.tile_order(W, H, 1, 3)
    own = np.zeros((H, W), bool)
    own[xy >> 16, xy & 0xFFFF] = True
    r = hipmod.Renderer(0, rank=1, world_size=3)
    try:
        prepare(r, rpt, "room", 1)
        r.render(SPP)
        got, _ = r.read_accum()
        assert own.any() and same_words(got[own], acc[own]) and not got[~own].any()
    finally:
        r.close()


def test_three_ranks_on_one_device(hipmod, rpt, oracle):
    """rpt_multi_set_punctual_lights: the gathered image is the restatement's, the counters sum to its"""
    acc, _, st = reference(oracle, "room", 2)
    w, rec, skybox, _ = model_scenes.scene("room")
    m = hipmod.MultiRenderer([0, 0, 0], allow_shared_device=True)
    try:
        m.upload_scene(w, skybox_f32=skybox)
        m.set_material_models(rec)
        m.set_punctual_lights(lights_ref.lights("room"), SHARE)
        m.set_config(model_scenes.config("room", 2, W, H))
        m.reset(rpt.blue_noise_seeds(W, H))
        m.render(SPP)
        got, n = m.read_accum()
        assert n == SPP and same_words(got, acc)
        counters_match(m.stats(), st)
    finally:
        m.close()


def _run(r, rpt, name, nee, lts, force=False):
    prepare(r, rpt, name, nee, lts=lts)
    r.debug_force_punctual_kernels(force)
    before = launches(r)
    try:
        r.render(SPP)
    finally:
        r.debug_force_punctual_kernels(False)
    gs = r.stats()
    d = {k: v - before[k] for k, v in gs["kernel_launches"].items()}
    return (r.read_accum()[0].copy(), r.read_rng().copy(), [gs[k] for k in ("extension_rays", "shadow_rays", "sky_evals", "shadow_rays_elided")], d,
            r.debug_last_shade_variant())


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("name", ["room", "open", "textured"])
def test_without_nee_the_lights_change_nothing(variants, rpt, oracle, name, compact):
    """nee 0: no BSDF sample meets a delta light — bytes, counters, launches and the variant launched are those of the run without lights, forced or not"""
    r = variants(compact, 0)
    base = _run(r, rpt, name, 0, None)
    assert base[4] == SHADE_MODELS
    check_against(r, model_scenes.reference(oracle, name, 0, W, H, SPP))
    for lts, force in (("scene", False), ("scene", True), (None, True)):
        got = _run(r, rpt, name, 0, lts, force)
        assert same_words(got[0], base[0]) and np.array_equal(got[1], base[1]) and got[2:] == base[2:]


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("nee", [1, 2])
@pytest.mark.parametrize("name", ["room", "open", "textured"])
def test_the_forced_variant_without_lights_is_the_run_without_it(variants, rpt, oracle, name, nee, compact):
    """no lights through k_shade_punctual (q = 0: u = l1, the pdf times 1.0f): every output byte, counter and launch count of the models variant"""
    r = variants(compact, 0)
    base = _run(r, rpt, name, nee, None)
    assert base[4] == SHADE_MODELS
    check_against(r, model_scenes.reference(oracle, name, nee, W, H, SPP))
    got = _run(r, rpt, name, nee, None, force=True)
    assert got[4] == SHADE_PUNCTUAL
    assert same_words(got[0], base[0]) and np.array_equal(got[1], base[1]) and got[2] == base[2] and got[3] == base[3]


def _plain_scene(rpt, world, which):
    if which == "DarkCornell":
        return world("DarkCornell"), None, {}
    w, skybox = scenes.textured_scene()
    return w, skybox, dict(has_skybox=1, cam_position=(0.0, 1.8, -1.8, 0.0), cam_rotation=(0.15, 0.0, 0.0, 0.0))


@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("which", ["DarkCornell", "textured"])
def test_a_context_that_never_set_lights_renders_as_before(hipmod, rpt, oracle, world, which, nee):
    """the existing scenes on a context that never heard of the lights: the oracle's bytes through k_shade; and, forced through k_shade_punctual (NEE only)
    with no records of any kind, the same bytes and launches"""
    w, skybox, view = _plain_scene(rpt, world, which)
    cfg, seeds = rpt.default_config(W, H, nee=nee, **view), rpt.blue_noise_seeds(W, H)
    ref, ref_rng, ref_st = oracle.trace_cpu(cfg, oracle.scene(w, skybox_f32=skybox), seeds, SPP)
    r = hipmod.Renderer(0)
    try:
        seen = []
        for force in (False, True):
            r.upload_scene(w, skybox_f32=skybox)
            assert len(r.punctual_lights()[0]) == 0 and r.punctual_lights()[1] == 0.0
            r.debug_force_punctual_kernels(force)
            r.set_config(cfg)
            r.reset(seeds)
            before = launches(r)
            r.render(SPP)
            got, n = r.read_accum()
            assert n == SPP and same_words(got, ref) and np.array_equal(r.read_rng().reshape(-1), np.asarray(ref_rng).reshape(-1))
            gs = r.stats()
            assert (gs["extension_rays"], gs["shadow_rays"], gs["sky_evals"]) == (ref_st.extension_rays, ref_st.shadow_rays, ref_st.sky_evals)
            assert r.debug_last_shade_variant() == (SHADE_PUNCTUAL if force and nee != 0 else SHADE)
            seen.append({k: v - before[k] for k, v in gs["kernel_launches"].items()})
        assert seen[0] == seen[1]
    finally:
        r.close()


def test_life_cycle_of_the_lights(variants, rpt, oracle):
    """cleared by (NULL, 0) and by rpt_upload_scene, kept by rpt_set_config; a cleared context renders the image without lights again"""
    r = variants()
    w, rec, skybox, _ = model_scenes.scene("room")
    lts = lights_ref.lights("room")
    seeds = rpt.blue_noise_seeds(W, H)
    r.set_camera_lens(None)
    r.upload_scene(w, skybox_f32=skybox)
    assert len(r.punctual_lights()[0]) == 0                # a new scene has none
    r.set_material_models(rec)
    r.set_punctual_lights(lts, 0.25)
    got, q = r.punctual_lights()
    assert got.tobytes() == lts.tobytes() and q == 0.25     # the round trip
    r.set_punctual_lights(lts, SHARE)
    r.set_config(model_scenes.config("room", 0, W, H))
    r.set_config(model_scenes.config("room", 1, W, H))     # the lights survive rpt_set_config
    assert r.punctual_lights()[0].tobytes() == lts.tobytes() and r.punctual_lights()[1] == F(SHARE)
    r.reset(seeds)
    r.render(SPP)
    check_against(r, reference(oracle, "room", 1))
    r.set_punctual_lights(None)                            # none again
    assert len(r.punctual_lights()[0]) == 0 and r.punctual_lights()[1] == 0.0 and np.array_equal(r.material_models(), rec)
    r.reset(seeds)
    r.render(SPP)
    assert r.debug_last_shade_variant() == SHADE_MODELS
    check_against(r, model_scenes.reference(oracle, "room", 1, W, H, SPP))
    r.set_punctual_lights(lts[:1], SHARE)                  # one light, between two batches: the caller resets
    r.reset(seeds)
    r.render(SPP)
    assert r.debug_last_shade_variant() == SHADE_PUNCTUAL
    check_against(r, reference(oracle, "room", 1, lts=lts[:1]))
    r.upload_scene(w, skybox_f32=skybox)                   # rpt_upload_scene clears them
    assert len(r.punctual_lights()[0]) == 0 and r.punctual_lights()[1] == 0.0


def test_refusals_leave_the_context_as_it_was(hipmod, rpt, oracle):
    w, rec, skybox, _ = model_scenes.scene("room")
    lts = lights_ref.lights("room")
    r = hipmod.Renderer(0)
    try:
        with pytest.raises(hipmod.RptError) as e:          # before a scene
            r.set_punctual_lights(lts, SHARE)
        assert e.value.code == -1
        prepare(r, rpt, "room", 1)

        def refused(records, share, *words):
            with pytest.raises(hipmod.RptError) as e:
                r.set_punctual_lights(records, share)
            assert e.value.code == -1
            for word in words:
                assert word in str(e.value), str(e.value)
            got, q = r.punctual_lights()
            assert got.tobytes() == lts.tobytes() and q == F(SHARE)

        def with_(index, field, value):
            bad = lts.copy()
            bad[field][index] = value
            return bad

        refused(with_(1, "type", 3), SHARE, "record 1")                                        # a type above 2
        for field in ("position", "direction", "intensity"):
            for value in (np.nan, np.inf, -np.inf):
                refused(with_(2, field, (value, 0.0, 0.0)), SHARE, "record 2")                 # not finite
        refused(with_(0, "intensity", (1.0, -0.5, 1.0)), SHARE, "record 0")                    # a negative intensity
        refused(with_(1, "direction", (0.0, -1.01, 0.0)), SHARE, "record 1")                   # |len^2 - 1| > 1e-3 on a spot ...
        refused(with_(2, "direction", (0.0, 0.0, 0.0)), SHARE, "record 2")                     # ... and on a directional record
        r.set_punctual_lights(with_(0, "direction", (0.0, 5.0, 0.0)), SHARE)                   # (a point light's direction is ignored)
        r.set_punctual_lights(lts, SHARE)
        for field in ("angle_scale", "angle_offset"):
            refused(with_(1, field, np.nan), SHARE, "record 1")
            refused(with_(1, field, np.inf), SHARE, "record 1")
        bad = lts.copy(); bad["reserved"][2, 3] = 1; refused(bad, SHARE, "record 2")           # reserved != 0
        for share in (0.0, 1.0, -0.5, 1.5, np.nan):                                            # the room has emissive triangles: (0, 1) exclusive
            refused(lts, share, "pick_share")
        L = hipmod.lib()
        assert L.rpt_set_punctual_lights(r._h, None, len(lts), SHARE) == -1                    # NULL with n != 0 ...
        keep = np.ascontiguousarray(lts)
        assert L.rpt_set_punctual_lights(r._h, hipmod.ptr(keep), 0, SHARE) == -1               # ... and the reverse
        many = np.repeat(lts[:1], 65536)
        refused(many, SHARE, "65535")
        got, q = r.punctual_lights()
        assert got.tobytes() == lts.tobytes() and q == F(SHARE)
        r.render(SPP)                                                                          # the next render is unaffected
        check_against(r, reference(oracle, "room", 1))
        prepare(r, rpt, "open", 1, share=7.0)                                                  # no emissive triangle: pick_share is ignored, q = 1
        assert r.punctual_lights()[1] == 1.0
    finally:
        r.close()
