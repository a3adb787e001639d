"""Material models on the device (rpt_set_material_models; csrc/rpt_models.hip k_shade_models): accumulators, rng and counters word for word against the
restatement tests/models_oracle, in both shade variants and both slot layouts, through every call shape and route into the pipeline; the forced variant
on all-PBR scenes against the plain kernels; life cycle, furnace and refusals.  80 x 72 (a whole tile, a 16-pixel and an 8-pixel remainder), 8 spp."""
import numpy as np
import pytest

import model_scenes
import scenes
from model_scenes import furnace_check, furnace_primary_miss, furnace_sky_value

pytestmark = pytest.mark.gpu

W, H, SPP = 80, 72, 8


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def reference(oracle, name, nee):
    return model_scenes.reference(oracle, name, nee, W, H, SPP)


def counters_match(gs, st):
    got = (gs["extension_rays"], gs["shadow_rays"], gs["sky_evals"], gs["shadow_rays_elided"])
    want = (st.extension_rays, st.shadow_rays, st.sky_evals, st.shadow_rays_zero_term)
    assert got == want, (got, want)


_renderers = {}


@pytest.fixture(scope="module")
def variants(hipmod):
    """one context per (RPT_SHADE_COMPACT, RPT_SLOT_Q_SHIFT): both are read by rpt_create"""
    import os

    def get(compact, q_shift):
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


def prepare(r, rpt, name, nee, records=True, **more):
    w, rec, skybox, _ = model_scenes.scene(name)
    r.upload_scene(w, skybox_f32=skybox)
    if records:
        r.set_material_models(rec)
    r.set_config(model_scenes.config(name, nee, W, H, **more))
    r.reset(rpt.blue_noise_seeds(W, H))
    return rec


def check_against(r, ref, counters=True):
    acc, rng, st = ref
    got, n = r.read_accum()
    assert n == SPP and same_words(got, acc)
    assert np.array_equal(r.read_rng().reshape(-1), np.asarray(rng).reshape(-1))
    if counters:
        counters_match(r.stats(), st)


@pytest.mark.parametrize("q_shift", [0, 5])
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("name", ["room", "open", "textured"])
def test_words_and_counters_are_the_restatements(variants, rpt, oracle, name, nee, compact, q_shift):
    r = variants(compact, q_shift)
    prepare(r, rpt, name, nee)
    r.render(SPP)                                        # a batch of known length: no slot takes a second sample
    check_against(r, reference(oracle, name, nee))


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("in_flight", [2, 1])
def test_slots_that_take_several_samples_and_one_slot_per_pixel(hipmod, rpt, oracle, compact, in_flight, monkeypatch):
    monkeypatch.setenv("RPT_SHADE_COMPACT", str(compact))
    r = hipmod.Renderer(0)
    try:
        r.set_samples_in_flight(in_flight)
        prepare(r, rpt, "room", 1)
        r.render(SPP)
        check_against(r, reference(oracle, "room", 1))
    finally:
        r.close()


def test_two_batches(variants, rpt, oracle):
    r = variants(0, 0)
    prepare(r, rpt, "room", 1)
    r.render(3)
    r.render(5)
    check_against(r, reference(oracle, "room", 1))


def test_moments_on(hipmod, rpt, oracle):
    r = hipmod.Renderer(0)
    try:
        r.set_moments(True)
        prepare(r, rpt, "room", 1)
        r.render(SPP)
        check_against(r, reference(oracle, "room", 1))
        assert np.all(r.read_moments()[..., 2] == SPP)
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
    acc, _, st = reference(oracle, "room", 1)
    w, rec, skybox, _ = model_scenes.scene("room")
    m = hipmod.MultiRenderer([0, 0, 0], allow_shared_device=True)
    try:
        m.upload_scene(w, skybox_f32=skybox)
        m.set_material_models(rec)
        m.set_config(model_scenes.config("room", 1, W, H))
        m.reset(rpt.blue_noise_seeds(W, H))
        m.render(SPP)
        got, n = m.read_accum()
        assert n == SPP and same_words(got, acc)
        counters_match(m.stats(), st)
    finally:
        m.close()


def _all_pbr_scene(rpt, world, which):
    if which == "DarkCornell":
        return world("DarkCornell"), None, {}
    w, skybox = scenes.textured_scene()
    return w, skybox, dict(has_skybox=1, cam_position=(0.0, 1.8, -1.8, 0.0), cam_rotation=(0.15, 0.0, 0.0, 0.0))


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("which", ["DarkCornell", "textured"])
def test_the_forced_variant_is_the_plain_kernels_on_an_all_pbr_scene(variants, rpt, world, which, nee, compact):
    """rpt_debug_force_model_kernels: image, rng and counters of k_shade_models equal k_shade's bit for bit, with no records and with records that say PBR"""
    w, skybox, view = _all_pbr_scene(rpt, world, which)
    r = variants(compact, 0)
    seeds = rpt.blue_noise_seeds(W, H)
    results = []
    try:
        for force, rec in ((False, None), (True, None), (True, model_scenes.records([0] * len(w.materials)))):
            r.upload_scene(w, skybox_f32=skybox)
            if rec is not None:
                r.set_material_models(rec)
            r.debug_force_model_kernels(force)
            r.set_config(rpt.default_config(W, H, nee=nee, **view))
            r.reset(seeds)
            r.render(SPP)
            gs = r.stats()
            results.append((r.read_accum()[0].copy(), r.read_rng().copy(), [gs[k] for k in ("extension_rays", "shadow_rays", "sky_evals", "shadow_rays_elided")]))
    finally:
        r.debug_force_model_kernels(False)
    for acc, rng, counters in results[1:]:
        assert same_words(acc, results[0][0]) and np.array_equal(rng, results[0][1]) and counters == results[0][2]


def test_life_cycle_of_the_records(variants, rpt, oracle):
    """cleared by (NULL, 0) and by rpt_upload_scene, kept by rpt_set_config; a cleared context renders the image it rendered before"""
    r = variants(0, 0)
    w, rec, skybox, _ = model_scenes.scene("room")
    seeds = rpt.blue_noise_seeds(W, H)
    r.upload_scene(w, skybox_f32=skybox)
    assert len(r.material_models()) == 0                 # a new scene has none
    r.set_config(model_scenes.config("room", 1, W, H))
    r.reset(seeds)
    r.render(SPP)
    plain = r.read_accum()[0].copy()
    r.set_material_models(rec)
    assert np.array_equal(r.material_models(), rec)
    r.set_config(model_scenes.config("room", 0, W, H))
    r.set_config(model_scenes.config("room", 1, W, H))   # the records survive rpt_set_config
    assert np.array_equal(r.material_models(), rec)
    r.reset(seeds)
    r.render(SPP)
    check_against(r, reference(oracle, "room", 1))
    r.set_material_models(None)                          # every material PBR again
    assert len(r.material_models()) == 0
    r.reset(seeds)
    r.render(SPP)
    assert same_words(r.read_accum()[0], plain)
    r.set_material_models(rec)
    r.upload_scene(w, skybox_f32=skybox)                 # rpt_upload_scene clears them
    assert len(r.material_models()) == 0
    r.reset(seeds)
    r.render(SPP)
    assert same_words(r.read_accum()[0], plain)


def test_setting_records_between_batches_leaves_the_accumulator(variants, rpt, oracle):
    """as rpt_set_shadow_mode: accumulator, rng and statistics stay; the next batch takes the records"""
    r = variants(0, 0)
    prepare(r, rpt, "room", 1, records=False)
    r.render(3)
    before, rng_before, stats_before = r.read_accum()[0].copy(), r.read_rng().copy(), r.stats()
    r.set_material_models(model_scenes.scene("room")[1])
    assert same_words(r.read_accum()[0], before) and np.array_equal(r.read_rng(), rng_before)
    assert r.stats()["extension_rays"] == stats_before["extension_rays"] and r.read_accum()[1] == 3
    r.render(5)
    assert r.read_accum()[1] == 8 and not same_words(r.read_accum()[0], before)


@pytest.mark.parametrize("compact", [0, 1])
def test_furnace_on_the_device(variants, rpt, oracle, compact):
    r = variants(compact, 0)
    prepare(r, rpt, "furnace", 0)
    r.render(SPP)
    acc, n = r.read_accum()
    assert n == SPP
    furnace_check(acc, furnace_sky_value(oracle, W, H), furnace_primary_miss(model_scenes.config("furnace", 0, W, H)), SPP)
    check_against(r, reference(oracle, "furnace", 0))


def test_refusals_leave_the_context_as_it_was(hipmod, rpt, oracle):
    w, rec, skybox, _ = model_scenes.scene("room")
    r = hipmod.Renderer(0)
    try:
        with pytest.raises(hipmod.RptError) as e:        # before a scene
            r.set_material_models(rec)
        assert e.value.code == -1
        prepare(r, rpt, "room", 1)

        def refused(records):
            with pytest.raises(hipmod.RptError) as e:
                r.set_material_models(records)
            assert e.value.code == -1
            assert np.array_equal(r.material_models(), rec)

        bad = rec.copy(); bad["model"][1] = 3; refused(bad)                               # a model above 2
        for ior in (0.0, -1.5, np.inf, np.nan):                                           # an ior that is not finite or not above 0, on a GLASS record
            bad = rec.copy(); bad["ior"][3] = ior; refused(bad)
        refused(rec[:-1]); refused(np.concatenate([rec, rec[:1]]))                        # a wrong count
        ok = rec.copy(); ok["ior"][0] = np.nan; ok["ior"][1] = -1.0                       # ... ignored on the others
        r.set_material_models(ok)
        r.set_material_models(rec)
        r.render(SPP)                                                                     # the next render is unaffected
        check_against(r, reference(oracle, "room", 1))
    finally:
        r.close()
