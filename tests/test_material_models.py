"""Material models without a GPU: the bit-exact restatement tests/models_oracle (the reference's trace_pixel with the model switch at lib.rs:144) against the
oracle where every record is PBR, and the furnace statement, which needs no reference."""
import numpy as np
import pytest

import model_scenes
import scenes


def _darkcornell(rpt, world):
    return world("DarkCornell"), None, {}


def _textured(rpt, world):
    w, skybox = scenes.textured_scene()
    return w, skybox, dict(has_skybox=1, cam_position=(0.0, 1.8, -1.8, 0.0), cam_rotation=(0.15, 0.0, 0.0, 0.0))


@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("which", ["DarkCornell", "textured"])
def test_all_pbr_records_give_the_oracles_words_and_counters(rpt, oracle, world, which, nee):
    """the restated frame is the oracle's: 64 x 48 x 4 spp, with records that say PBR and with none"""
    w, skybox, view = (_darkcornell if which == "DarkCornell" else _textured)(rpt, world)
    W, H, spp = 64, 48, 4
    cfg = rpt.default_config(W, H, nee=nee, **view)
    seeds = rpt.blue_noise_seeds(W, H)
    sc = oracle.scene(w, skybox_f32=skybox)
    ref, ref_rng, ref_st = oracle.trace_cpu(cfg, sc, seeds, spp)
    for rec in (model_scenes.records([model_scenes.MODEL_PBR] * len(w.materials)), None):
        acc, rng, st = model_scenes.models_trace_cpu(cfg, sc, rec, seeds, spp)
        assert np.array_equal(acc.view(np.uint32), ref.view(np.uint32))
        assert np.array_equal(rng, ref_rng)
        assert (st.samples, st.extension_rays, st.shadow_rays, st.sky_evals, st.light_index_clamped) == \
               (ref_st.samples, ref_st.extension_rays, ref_st.shadow_rays, ref_st.sky_evals, ref_st.light_index_clamped)
    if nee:
        dead = oracle.dead_shadow_rays(cfg, sc, seeds, spp)
        assert (st.shadow_rays, st.shadow_rays_zero_term) == dead[:2]          # the zero-term count is the oracle's own analysis hook's


def test_furnace_every_sample_is_the_sky_or_nothing(rpt, oracle):
    W, H, spp = 32, 24, 8
    acc, _, st = model_scenes.reference(oracle, "furnace", 0, W, H, spp)
    miss = model_scenes.furnace_primary_miss(model_scenes.config("furnace", 0, W, H))
    assert miss.any() and not miss.all()
    k = model_scenes.furnace_check(acc, model_scenes.furnace_sky_value(oracle, W, H), miss, spp)
    assert (k[~miss] == spp).any()                        # paths through the glass reach the sky too
    assert st.shadow_rays == 0


def test_the_records_of_the_binding_are_the_headers(hipmod):
    assert hipmod.MATERIAL_MODEL_DTYPE.itemsize == 16 and hipmod.MATERIAL_MODEL_DTYPE.fields["ior"][1] == 4
    assert hipmod.MATERIAL_MODEL_DTYPE == model_scenes.MATERIAL_MODEL_DTYPE
    rec = hipmod.material_models([hipmod.MODEL_PBR, hipmod.MODEL_GLASS, hipmod.MODEL_LAMBERTIAN], [0.0, 1.33, 0.0])
    assert rec["model"].tolist() == [0, 2, 1] and rec["ior"][1] == np.float32(1.33)


@pytest.mark.parametrize("name", ["room", "open", "textured"])
def test_the_models_change_the_image_and_stay_finite(rpt, oracle, name):
    """the scenes do what they are for: with the records the restatement's image is finite and differs from the all-PBR one; Glass hits sample no light"""
    W, H, spp = 32, 24, 2
    w, rec, skybox, _ = model_scenes.scene(name)
    for nee in (0, 1):
        acc, _, st = model_scenes.reference(oracle, name, nee, W, H, spp)
        assert np.isfinite(acc).all()
        cfg = model_scenes.config(name, nee, W, H)
        plain, _, plain_st = model_scenes.models_trace_cpu(cfg, oracle.scene(w, skybox_f32=skybox), None, rpt.blue_noise_seeds(W, H), spp)
        assert not np.array_equal(acc, plain)
        if nee and name != "open":                          # (the open scene has no emitter: no light is ever sampled)
            assert 0 < st.shadow_rays != plain_st.shadow_rays


def _glass_glb(path):
    """one triangle and four materials: plain, transmissive without and with KHR_materials_ior, and transmissionFactor 0"""
    materials = [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.7, 0.6, 1.0]}},
                 {"extensions": {"KHR_materials_transmission": {"transmissionFactor": 1.0}}},
                 {"extensions": {"KHR_materials_transmission": {"transmissionFactor": 0.25}, "KHR_materials_ior": {"ior": 1.33}}},
                 {"extensions": {"KHR_materials_transmission": {"transmissionFactor": 0.0}, "KHR_materials_ior": {"ior": 2.0}}}]
    return scenes.write_glb(str(path), [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [0, 1, 2], materials=materials)


def test_the_loader_reads_transmission_and_ior_only_when_asked(rpt, tmp_path):
    path = _glass_glb(tmp_path / "glass.glb")
    plain, flagged = rpt.World.from_path(path), rpt.World.from_path(path, material_models=True)
    assert len(plain.material_models) == len(plain.materials) == 4 and not plain.material_models["model"].any()
    assert flagged.material_models["model"].tolist() == [0, 2, 2, 0]
    assert flagged.material_models["ior"][1:3].tolist() == [np.float32(1.5), np.float32(1.33)]
    for field in ("per_vertex", "indices", "nodes", "materials", "light_pick"):      # the world itself does not depend on the flag
        assert getattr(plain, field).tobytes() == getattr(flagged, field).tobytes()
    a, b = tmp_path / "a.rptscene", tmp_path / "b.rptscene"
    plain.save(str(a)); flagged.save(str(b))
    assert a.read_bytes() == b.read_bytes()                                          # ... nor does the cache, which does not carry the records
    assert not rpt.World.from_cache(str(b)).material_models["model"].any()
