"""Absorbing glass on the device (rpt_set_material_volumes; csrc/rpt_volumes.hip k_shade_volumes): accumulators, rng and counters word for word against the
restatement tests/volume_oracle, in both shade variants and both slot layouts, through every call shape and route into the pipeline; records that absorb
nothing against the models run, byte for byte and launch for launch; the forced variant; life cycle and refusals.  80 x 72 (a whole tile, a 16-pixel and an
8-pixel remainder) and 37 x 23 (partial 8 x 8 blocks), 8 spp."""
import os

import numpy as np
import pytest

import lens_ref
import model_scenes
import moments_ref
import scenes
import volume_ref
from volume_ref import same_bits_or_both_nan, transmit_inputs

pytestmark = pytest.mark.gpu

W, H, SPP = 80, 72, 8
F = np.float32
SHADE, SHADE_MODELS, SHADE_VOLUMES = 0, 1, 2              # rpt_debug_last_shade_variant


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def reference(oracle, name, nee, size=(W, H), spp=SPP, lens=None, vols="scene"):
    return volume_ref.reference(oracle, name, nee, size[0], size[1], spp, lens=lens, vols=vols, **model_scenes.lens_overrides(nee, lens))


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


def prepare(r, rpt, name, nee, size=(W, H), lens=None, vols="scene", models=True, volumes_first=False):
    """scene, both record sets, configuration, lens, reset (the lens is taken off first: a context that holds an aperture refuses a 31-dimension configuration)"""
    w, rec, skybox, _ = model_scenes.scene(name)
    rec_v = volume_ref.volumes(name) if isinstance(vols, str) else vols
    r.set_camera_lens(None)
    r.debug_force_volume_kernels(False)
    r.upload_scene(w, skybox_f32=skybox)                      # (clears both record sets)
    if volumes_first and rec_v is not None:
        r.set_material_volumes(rec_v)
    if models:
        r.set_material_models(rec)
    if not volumes_first and rec_v is not None:
        r.set_material_volumes(rec_v)
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
    thr, sigma, t = transmit_inputs()
    assert same_bits_or_both_nan(variants().debug_volume_transmit(thr, sigma, t), hipmod.debug_volume_transmit_host(thr, sigma, t))


@pytest.mark.parametrize("q_shift", [0, 5])
@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("name", ["room", "small_room", "open", "textured"])
def test_words_and_counters_are_the_restatements(variants, rpt, oracle, name, nee, compact, q_shift):
    """small_room and textured live in LDS: the FIRST walk over prepared slots, and without NEE the LAST walk that ends the paths itself"""
    r = variants(compact, q_shift)
    prepare(r, rpt, name, nee)
    r.render(SPP)                                        # a batch of known length: no slot takes a second sample
    assert r.debug_last_shade_variant() == SHADE_VOLUMES
    ref = reference(oracle, name, nee)
    assert ref[2].segments_absorbed > 0
    check_against(r, ref)


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("nee", [0, 1])
@pytest.mark.parametrize("name", ["room", "textured"])
def test_an_image_of_partial_blocks(variants, rpt, oracle, name, nee, compact):
    r = variants(compact, 0)
    prepare(r, rpt, name, nee, size=(37, 23))
    r.render(SPP)
    check_against(r, reference(oracle, name, nee, size=(37, 23)))


def test_the_last_walk_ends_the_paths_of_the_small_room(hipmod, rpt, oracle):
    """a known-length batch without NEE in an LDS scene: the last iteration's walk ends the paths itself — nothing reads the throughput at the last bounce,
    so the rule has nothing to do there — and seven shade passes are launched, all of them k_shade_volumes"""
    r = hipmod.Renderer(0)
    try:
        prepare(r, rpt, "small_room", 0)
        assert r.last_bounce_order()["mode"] != 0
        before = launches(r)
        r.render(SPP)
        d = {k: v - before[k] for k, v in launches(r).items()}
        assert d["traverse"] == 8 and d["shade"] == 7, d
        assert r.debug_last_shade_variant() == SHADE_VOLUMES
        check_against(r, reference(oracle, "small_room", 0))
    finally:
        r.close()


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_two_batches_and_an_asynchronous_one(variants, rpt, oracle, name):
    r = variants()
    prepare(r, rpt, name, 1)
    r.render(3)
    r.render(5)
    check_against(r, reference(oracle, name, 1))
    r.reset(rpt.blue_noise_seeds(W, H))
    r.render_async(SPP)
    r.wait()
    check_against(r, reference(oracle, name, 1))


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("in_flight", [2, 1])
def test_the_polled_route_slots_that_take_several_samples(hipmod, rpt, oracle, compact, in_flight, monkeypatch):
    monkeypatch.setenv("RPT_SHADE_COMPACT", str(compact))
    r = hipmod.Renderer(0)
    try:
        r.set_samples_in_flight(in_flight)
        prepare(r, rpt, "room", 1)
        r.render(SPP)
        check_against(r, reference(oracle, "room", 1))
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


@pytest.mark.parametrize("in_flight,spp", [(None, SPP), (2, 5)])
def test_moments_on(hipmod, rpt, oracle, in_flight, spp):
    """the record equals tests/moments_ref.py over the restatement's per-sample radiances"""
    samples, _, _ = volume_ref.per_sample(oracle, "room", 1, W, H, SPP)
    want, acc = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    for k in range(spp):
        moments_ref.add_sample(want, samples[k])
        acc[..., :3] = acc[..., :3] + samples[k]
        acc[..., 3] = acc[..., 3] + F(1)
    r = hipmod.Renderer(0)
    try:
        if in_flight is not None:
            r.set_samples_in_flight(in_flight)
        r.set_moments(True)
        prepare(r, rpt, "room", 1)
        r.render(spp)
        if spp == SPP:
            check_against(r, reference(oracle, "room", 1))
        assert same_words(r.read_accum()[0], acc)
        assert same_words(r.read_moments(), want)
    finally:
        r.close()


@pytest.mark.parametrize("nee", [0, 1])
@pytest.mark.parametrize("name", ["room", "small_room"])
def test_a_lens_with_an_aperture(variants, rpt, oracle, name, nee):
    """"both" of tests/lens_ref.py, with model_scenes.APERTURE_OVERRIDES: k_generate_lens scatters the origins, the camera may start anywhere"""
    r = variants()
    try:
        prepare(r, rpt, name, nee, lens="both")
        r.render(SPP)
        check_against(r, reference(oracle, name, nee, lens="both"))
    finally:
        r.set_camera_lens(None)


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
    """rpt_multi_set_material_volumes: the gathered image is the restatement's, the counters sum to its"""
    acc, _, st = reference(oracle, "room", 1)
    w, rec, skybox, _ = model_scenes.scene("room")
    m = hipmod.MultiRenderer([0, 0, 0], allow_shared_device=True)
    try:
        m.upload_scene(w, skybox_f32=skybox)
        m.set_material_volumes(volume_ref.volumes("room"))
        m.set_material_models(rec)
        m.set_config(model_scenes.config("room", 1, W, H))
        m.reset(rpt.blue_noise_seeds(W, H))
        m.render(SPP)
        got, n = m.read_accum()
        assert n == SPP and same_words(got, acc)
        counters_match(m.stats(), st)
    finally:
        m.close()


def _run(r, rpt, name, nee, vols, force=False):
    prepare(r, rpt, name, nee, vols=vols)
    r.debug_force_volume_kernels(force)
    before = launches(r)
    try:
        r.render(SPP)
    finally:
        r.debug_force_volume_kernels(False)
    gs = r.stats()
    d = {k: v - before[k] for k, v in gs["kernel_launches"].items()}
    return (r.read_accum()[0].copy(), r.read_rng().copy(), [gs[k] for k in ("extension_rays", "shadow_rays", "sky_evals", "shadow_rays_elided")], d,
            r.debug_last_shade_variant())


@pytest.mark.parametrize("compact", [0, 1])
@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("name", ["room", "textured"])
def test_records_that_absorb_nothing_are_the_models_run(variants, rpt, oracle, name, nee, compact):
    """all-zero records, and records on materials that are not Glass only: the kernels launched (k_shade_models, launch for launch) and every output byte are
    those of the run without volume records; the forced variant with all-zero records gives the same bytes through k_shade_volumes"""
    r = variants(compact, 0)
    models = model_scenes.scene(name)[1]
    zeros = volume_ref.records(np.zeros((len(models), 3)))
    elsewhere = volume_ref.records(np.where((models["model"] != model_scenes.MODEL_GLASS)[:, None], (0.7, 0.2, 1.5), 0.0))
    assert elsewhere["sigma"].any()
    base = _run(r, rpt, name, nee, None)
    assert base[4] == SHADE_MODELS
    check_against(r, model_scenes.reference(oracle, name, nee, W, H, SPP))
    for vols, force, variant in ((zeros, False, SHADE_MODELS), (elsewhere, False, SHADE_MODELS), (zeros, True, SHADE_VOLUMES), (None, True, SHADE_VOLUMES),
                                 (elsewhere, True, SHADE_VOLUMES)):
        got = _run(r, rpt, name, nee, vols, force)
        assert same_words(got[0], base[0]) and np.array_equal(got[1], base[1]) and got[2] == base[2]
        assert got[3] == base[3] and got[4] == variant


def _plain_scene(rpt, world, which):
    if which == "DarkCornell":
        return world("DarkCornell"), None, {}
    w, skybox = scenes.textured_scene()
    return w, skybox, dict(has_skybox=1, cam_position=(0.0, 1.8, -1.8, 0.0), cam_rotation=(0.15, 0.0, 0.0, 0.0))


@pytest.mark.parametrize("nee", [0, 1])
@pytest.mark.parametrize("which", ["DarkCornell", "textured"])
def test_a_context_that_never_set_a_record_renders_as_before(hipmod, rpt, oracle, world, which, nee):
    """the existing scenes on a context that never heard of volumes: the oracle's bytes through k_shade; and, forced through k_shade_volumes with no records
    of either kind, the same bytes and launches"""
    w, skybox, view = _plain_scene(rpt, world, which)
    cfg, seeds = rpt.default_config(W, H, nee=nee, **view), rpt.blue_noise_seeds(W, H)
    ref, ref_rng, ref_st = oracle.trace_cpu(cfg, oracle.scene(w, skybox_f32=skybox), seeds, SPP)
    r = hipmod.Renderer(0)
    try:
        seen = []
        for force in (False, True):
            r.upload_scene(w, skybox_f32=skybox)
            assert len(r.material_volumes()) == 0
            r.debug_force_volume_kernels(force)
            r.set_config(cfg)
            r.reset(seeds)
            before = launches(r)
            r.render(SPP)
            got, n = r.read_accum()
            assert n == SPP and same_words(got, ref) and np.array_equal(r.read_rng().reshape(-1), np.asarray(ref_rng).reshape(-1))
            gs = r.stats()
            assert (gs["extension_rays"], gs["shadow_rays"], gs["sky_evals"]) == (ref_st.extension_rays, ref_st.shadow_rays, ref_st.sky_evals)
            assert r.debug_last_shade_variant() == (SHADE_VOLUMES if force else SHADE)
            seen.append({k: v - before[k] for k, v in gs["kernel_launches"].items()})
        assert seen[0] == seen[1]
    finally:
        r.close()


def test_life_cycle_of_the_records(variants, rpt, oracle):
    """cleared by (NULL, 0) and by rpt_upload_scene, kept by rpt_set_config; a cleared context renders the models image again"""
    r = variants()
    w, rec, skybox, _ = model_scenes.scene("room")
    vols = volume_ref.volumes("room")
    seeds = rpt.blue_noise_seeds(W, H)
    r.set_camera_lens(None)
    r.upload_scene(w, skybox_f32=skybox)
    assert len(r.material_volumes()) == 0                # a new scene has none
    r.set_material_models(rec)
    r.set_material_volumes(vols)
    assert np.array_equal(r.material_volumes(), vols) and np.array_equal(r.material_models(), rec)
    r.set_config(model_scenes.config("room", 0, W, H))
    r.set_config(model_scenes.config("room", 1, W, H))   # the records survive rpt_set_config
    assert np.array_equal(r.material_volumes(), vols)
    r.reset(seeds)
    r.render(SPP)
    check_against(r, reference(oracle, "room", 1))
    r.set_material_volumes(None)                         # none again
    assert len(r.material_volumes()) == 0 and np.array_equal(r.material_models(), rec)
    r.reset(seeds)
    r.render(SPP)
    assert r.debug_last_shade_variant() == SHADE_MODELS
    check_against(r, model_scenes.reference(oracle, "room", 1, W, H, SPP))
    r.set_material_volumes(vols)
    r.set_material_models(None)                          # no Glass left: the volume records stay, stored and ignored
    assert np.array_equal(r.material_volumes(), vols)
    r.reset(seeds)
    r.render(SPP)
    assert r.debug_last_shade_variant() == SHADE
    r.set_material_models(rec)                           # ... and count again when the Glass records come back
    r.reset(seeds)
    r.render(SPP)
    assert r.debug_last_shade_variant() == SHADE_VOLUMES
    check_against(r, reference(oracle, "room", 1))
    r.upload_scene(w, skybox_f32=skybox)                 # rpt_upload_scene clears them
    assert len(r.material_volumes()) == 0 and len(r.material_models()) == 0


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_the_order_of_the_setters_does_not_matter(variants, rpt, oracle, name):
    r = variants()
    seen = []
    for volumes_first in (False, True):
        prepare(r, rpt, name, 1, volumes_first=volumes_first)
        before = launches(r)
        r.render(SPP)
        check_against(r, reference(oracle, name, 1))
        seen.append(({k: v - before[k] for k, v in launches(r).items()}, r.debug_last_shade_variant()))
    assert seen[0] == seen[1] and seen[0][1] == SHADE_VOLUMES


def test_setting_records_between_batches_leaves_the_accumulator(variants, rpt, oracle):
    """as rpt_set_material_models: accumulator, rng, statistics and the guides stay; the next batch takes the records"""
    r = variants()
    prepare(r, rpt, "room", 1, vols=None)
    r.render(3)
    before, rng_before, stats_before = r.read_accum()[0].copy(), r.read_rng().copy(), r.stats()
    r.set_material_volumes(volume_ref.volumes("room"))
    assert same_words(r.read_accum()[0], before) and np.array_equal(r.read_rng(), rng_before)
    assert r.stats()["extension_rays"] == stats_before["extension_rays"] and r.read_accum()[1] == 3
    r.render(5)
    assert r.read_accum()[1] == 8 and r.debug_last_shade_variant() == SHADE_VOLUMES
    mixed = r.read_accum()[0].copy()
    assert not same_words(mixed, before)
    assert not same_words(mixed, model_scenes.reference(oracle, "room", 1, W, H, SPP)[0])      # the last five samples absorbed


def test_refusals_leave_the_context_as_it_was(hipmod, rpt, oracle):
    w, rec, skybox, _ = model_scenes.scene("room")
    vols = volume_ref.volumes("room")
    r = hipmod.Renderer(0)
    try:
        with pytest.raises(hipmod.RptError) as e:        # before a scene
            r.set_material_volumes(vols)
        assert e.value.code == -1
        prepare(r, rpt, "room", 1)

        def refused(records, *words):
            with pytest.raises(hipmod.RptError) as e:
                r.set_material_volumes(records)
            assert e.value.code == -1
            for word in words:
                assert word in str(e.value), str(e.value)
            assert np.array_equal(r.material_volumes(), vols) and np.array_equal(r.material_models(), rec)

        for bad_sigma in (-0.5, np.nan, np.inf, -np.inf):                                 # a sigma channel that is negative, NaN or infinite
            bad = vols.copy(); bad["sigma"][2, 1] = bad_sigma; refused(bad, "record 2")     # (on any material: the records are checked before they are stored)
        bad = vols.copy(); bad["reserved"][4] = 1; refused(bad, "record 4")               # reserved != 0
        refused(vols[:-1]); refused(np.concatenate([vols, vols[:1]]))                     # a wrong count
        L = hipmod.lib()
        assert L.rpt_set_material_volumes(r._h, None, len(vols)) == -1                     # NULL with n != 0 ...
        keep = np.ascontiguousarray(vols)
        assert L.rpt_set_material_volumes(r._h, hipmod.ptr(keep), 0) == -1                 # ... and the reverse
        assert np.array_equal(r.material_volumes(), vols) and np.array_equal(r.material_models(), rec)
        r.render(SPP)                                                                     # the next render is unaffected
        check_against(r, reference(oracle, "room", 1))
    finally:
        r.close()
