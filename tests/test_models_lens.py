"""Material models under a camera lens without a GPU: the restatement with BOTH switches (tests/models_oracle models_lens_trace_cpu — the model at
lib.rs:144, the lens at lib.rs:38-51 through tests/lens_oracle/lens_camera.h) held from both sides word for word — under the default record it is the
models restatement, with every record PBR it is the lens restatement — and the furnace statement, which needs no reference, under a lens.  The device is
held to it bit for bit in tests/test_gpu_models_lens.py, the float64 second opinion is in tests/test_f64_models.py."""
import numpy as np
import pytest

import lens_ref
import model_scenes
from lens_ref import F, LENSES

W, H, SPP = 40, 36, 4


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def counters(st):
    return (st.samples, st.extension_rays, st.shadow_rays, st.sky_evals, st.light_index_clamped, st.shadow_rays_zero_term)


@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("name", ["room", "small_room", "open", "textured"])
def test_the_default_record_is_the_models_restatement_word_for_word(rpt, oracle, name, nee):
    """{1, 0, 1, 0}, and an inactive record with another focus: accumulator, rng and every counter of models_trace_cpu, under the 31-dimension configurations"""
    w, rec, skybox, _ = model_scenes.scene(name)
    cfg, sc, seeds = model_scenes.config(name, nee, W, H), oracle.scene(w, skybox_f32=skybox), rpt.blue_noise_seeds(W, H)
    want_acc, want_rng, want = model_scenes.models_trace_cpu(cfg, sc, rec, seeds, SPP)
    for record in ((1.0, 0.0, 1.0), (1.0, 0.0, 7.5)):
        acc, rng, st = model_scenes.models_lens_trace_cpu(cfg, sc, rec, lens_ref.lens(record), seeds, SPP)
        assert same_words(acc, want_acc) and np.array_equal(rng, want_rng)
        assert counters(st) == counters(want)


@pytest.mark.parametrize("nee", [0, 1])       # none, MIS
@pytest.mark.parametrize("which", ["DarkCornell", "textured"])
@pytest.mark.parametrize("lens_name", sorted(LENSES))
def test_all_pbr_records_are_the_lens_restatement_word_for_word(rpt, oracle, world, which, nee, lens_name):
    """no records, and records that all say PBR: accumulator, rng and every counter of lens_trace_cpu, for every lens"""
    w, skybox, _ = lens_ref.scene_and_view(world, which)
    cfg, sc, seeds = lens_ref.config(world, which, nee, W, H), oracle.scene(w, skybox_f32=skybox), rpt.blue_noise_seeds(W, H)
    want_acc, want_rng, want = lens_ref.lens_trace_cpu(cfg, sc, lens_ref.lens(lens_name), seeds, SPP)
    for rec in (None, model_scenes.records([model_scenes.MODEL_PBR] * len(w.materials))):
        acc, rng, st = model_scenes.models_lens_trace_cpu(cfg, sc, rec, lens_ref.lens(lens_name), seeds, SPP)
        assert same_words(acc, want_acc) and np.array_equal(rng, want_rng)
        assert counters(st) == counters(want)


@pytest.mark.parametrize("lens_name", ["fov", "narrow"])
def test_a_lens_without_an_aperture_leaves_entry_31_to_the_path(rpt, oracle, lens_name):
    """under the 31-dimension configurations the path draws table entry 31 (a roulette) while the lens does not read it: the restatement raises no flag, and
    the image differs from the one under the 30-dimension configuration, which differs only in that draw"""
    acc31, _, st31 = model_scenes.reference(oracle, "room", 0, W, H, SPP, lens=lens_name)
    acc30, _, st30 = model_scenes.reference(oracle, "room", 0, W, H, SPP, lens=lens_name, **model_scenes.APERTURE_OVERRIDES[0])
    assert st31.error_flags == 0 and st30.error_flags == 0
    assert not same_words(acc31, acc30) and st31.extension_rays != st30.extension_rays


def test_an_aperture_with_31_dimensions_is_flagged_by_the_restatement(rpt, oracle):
    """what rpt_set_camera_lens refuses with RPT_ECONFIG: a path that draws entry 31 shares it with the lens sample; the overrides of model_scenes keep clear"""
    w, rec, skybox, _ = model_scenes.scene("room")
    sc, seeds = oracle.scene(w, skybox_f32=skybox), rpt.blue_noise_seeds(W, H)
    for nee in (0, 1, 2):
        with pytest.raises(AssertionError):
            model_scenes.models_lens_trace_cpu(model_scenes.config("room", nee, W, H), sc, rec, lens_ref.lens("both"), seeds, SPP)
        cfg = model_scenes.config("room", nee, W, H, **model_scenes.lens_overrides(nee, "both"))
        model_scenes.models_lens_trace_cpu(cfg, sc, rec, lens_ref.lens("both"), seeds, 1)
    assert model_scenes.lens_overrides(0, "fov") == {} and model_scenes.lens_overrides(1, None) == {}


@pytest.mark.parametrize("lens_name", ["both", "fov"])
def test_one_pixel_sample_is_the_image_loops(rpt, oracle, lens_name):
    """models_lens_trace_pixel against one-sample passes of models_lens_trace_cpu, chosen pixels of the room under MIS"""
    nee = 1
    w, rec, skybox, _ = model_scenes.scene("room")
    cfg = model_scenes.config("room", nee, W, H, **model_scenes.lens_overrides(nee, lens_name))
    sc, seeds = oracle.scene(w, skybox_f32=skybox), rpt.blue_noise_seeds(W, H)
    samples = model_scenes.per_sample_radiances(oracle, "room", nee, W, H, 2, lens=lens_name, **model_scenes.lens_overrides(nee, lens_name))
    flat = np.asarray(seeds).reshape(-1)
    for x, y in ((0, 0), (W - 1, 0), (W // 2, H // 2), (7, H - 1), (W - 1, H - 1), (13, 20)):
        s = flat[y * W + x]
        for k in range(2):
            got, flags = model_scenes.models_lens_trace_pixel(cfg, sc, rec, lens_ref.lens(lens_name), x, y, int(s["n"]) + k, int(s["offset"]))
            assert flags == 0 and same_words(got, samples[k, y, x])


@pytest.mark.parametrize("lens_name", ["fov", "aperture", "both"])
def test_furnace_under_a_lens_every_sample_is_the_sky_or_nothing(rpt, oracle, lens_name):
    """Under any camera: Glass of albedo 1 under a constant sky, so every sample is exactly the sky's f32 value or 0.  The primary-miss mask of
    model_scenes.furnace_primary_miss is the reference camera's; here it comes from the restatement's own rays (lens_ref.lens_rays is the same
    lens_camera_ray): a pixel whose eight rays all pass the unit sphere at (0, 0, 3) by a margin takes the sky eight times."""
    W, H, spp = 32, 24, 8
    more = model_scenes.lens_overrides(0, lens_name)
    acc, rng, st = model_scenes.reference(oracle, "furnace", 0, W, H, spp, lens=lens_name, **more)
    s = model_scenes.furnace_sky_value(oracle, W, H)
    k = model_scenes.furnace_check(acc, s, None, spp)
    assert st.shadow_rays == 0 and (k == spp).any()

    cfg = model_scenes.config("furnace", 0, W, H, **more)
    seeds = np.asarray(rpt.blue_noise_seeds(W, H)).reshape(-1)
    keys = seeds["n"].astype(np.uint64) + seeds["offset"].astype(np.uint64)      # lens_rays takes a key as n with offset 0: a draw reads n + offset alone
    ys, xs = np.divmod(np.arange(W * H), W)
    miss = np.ones(W * H, bool)
    for j in range(spp):
        o, d = lens_ref.lens_rays(cfg, lens_ref.lens(lens_name), (xs | (ys << 16)).astype(np.uint32), ((keys + np.uint64(j)) & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        to = np.array([0.0, 0.0, 3.0]) - o.astype(np.float64)
        along = (to * d).sum(-1)
        miss &= (to * to).sum(-1) - along * along > 1.0 + 0.05
    miss = miss.reshape(H, W)
    assert miss.any() and not miss.all()
    assert np.all(k[miss] == spp)
