"""Absorbing glass without a GPU (include/rpt/rpt.h rpt_set_material_volumes): the bit-exact restatement tests/volume_oracle against the models restatement
where no record absorbs, the arithmetic of csrc/k_volume.h in the host build against a numpy float32 restatement, the scenes of tests/volume_ref.py doing
what they are for, the furnace statements, which need no reference, and the loader."""
import numpy as np
import pytest

import lens_ref
import model_scenes
import scenes
import volume_ref

W, H = 32, 24


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("lens_name", [None, "both"])
@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("name", ["room", "textured"])
def test_without_absorption_the_restatement_is_the_models_restatement(rpt, oracle, name, nee, lens_name):
    """no volume records, and all-zero records: accumulators, rng and counters of models_lens_trace_cpu word for word, with and without a lens"""
    spp = 2
    w, rec, skybox, _ = model_scenes.scene(name)
    cfg = model_scenes.config(name, nee, W, H, **model_scenes.lens_overrides(nee, lens_name))
    sc, seeds, lens = oracle.scene(w, skybox_f32=skybox), rpt.blue_noise_seeds(W, H), lens_ref.lens(lens_name)
    ref, ref_rng, ref_st = model_scenes.models_lens_trace_cpu(cfg, sc, rec, lens, seeds, spp)
    for vols in (None, volume_ref.records(np.zeros((len(rec), 3)))):
        acc, rng, st = volume_ref.volume_lens_trace_cpu(cfg, sc, rec, vols, lens, seeds, spp)
        assert np.array_equal(words(acc), words(ref))
        assert np.array_equal(rng, ref_rng)
        assert (st.samples, st.extension_rays, st.shadow_rays, st.sky_evals, st.light_index_clamped, st.shadow_rays_zero_term) == \
               (ref_st.samples, ref_st.extension_rays, ref_st.shadow_rays, ref_st.sky_evals, ref_st.light_index_clamped, ref_st.shadow_rays_zero_term)
        assert st.segments_absorbed == 0


def expr_f32(x):
    """rptm::expr as rpt_math.h states it: NaN passes, above 89 +inf, below -104 +0, else exp correctly rounded to float32 (float64's exp rounded once)"""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        mid = np.exp(np.clip(x.astype(np.float64), -104.0, 89.0)).astype(np.float32)
    out = np.where(x > np.float32(89.0), np.float32(np.inf), np.where(x < np.float32(-104.0), np.float32(0.0), mid))
    return np.where(np.isnan(x), x, out).astype(np.float32)


def vol_transmit_f32(throughput, sigma, t):
    """csrc/k_volume.h vol_transmit in numpy float32: T_c = expr(-(sigma_c * t)), an f32 product, then negate; throughput * T"""
    throughput, sigma, t = np.asarray(throughput, np.float32), np.asarray(sigma, np.float32), np.asarray(t, np.float32)
    with np.errstate(all="ignore"):
        product = sigma * t[:, None]
        assert product.dtype == np.float32
        return throughput * expr_f32(-product)


def test_the_host_build_of_vol_transmit_is_its_float32_restatement(hipmod):
    thr, sigma, t = volume_ref.transmit_inputs()
    got, want = hipmod.debug_volume_transmit_host(thr, sigma, t), vol_transmit_f32(thr, sigma, t)
    assert volume_ref.same_bits_or_both_nan(got, want), np.argwhere(words(got) != words(want))
    assert np.array_equal(words(got[0]), words(thr[0]))                       # t = 0: T = 1, the throughput bit for bit
    assert words(got[1, 1]) == words(thr[1, 1]) and got[1, 0] < thr[1, 0]      # sigma = 0 in one channel leaves that channel
    assert np.array_equal(words(got[2, :2]), words(np.zeros(2, np.float32)))   # an overflowing product: T = +0
    assert np.array_equal(words(got[3]), words(thr[3]))                        # a denormal product: T = 1
    assert np.isnan(got[4, 0]) and got[4, 1] == 0.0 and np.isinf(got[4, 2])    # inf * 0 is NaN, as the pipeline passes it; sigma = 0 keeps the inf


def test_the_records_of_the_binding_are_the_headers(hipmod):
    assert hipmod.MATERIAL_VOLUME_DTYPE.itemsize == 16 and hipmod.MATERIAL_VOLUME_DTYPE.fields["reserved"][1] == 12
    assert hipmod.MATERIAL_VOLUME_DTYPE == volume_ref.MATERIAL_VOLUME_DTYPE
    rec = hipmod.material_volumes([(0.0, 0.0, 0.0), (0.8, 0.3, 0.1)])
    assert rec["sigma"].tolist() == [[0.0, 0.0, 0.0], [np.float32(0.8), np.float32(0.3), np.float32(0.1)]] and not rec["reserved"].any()
    s = hipmod.absorption((0.5, 1.0, 0.0), 2.0)
    assert s.dtype == np.float32 and s[0] == np.float32(np.log(2.0) / 2.0) and words(s[1]) == 0 and s[2] == np.finfo(np.float32).max


@pytest.mark.parametrize("nee", [0, 1])
@pytest.mark.parametrize("name", ["room", "small_room", "open", "textured"])
def test_the_scenes_absorb(oracle, name, nee, capsys):
    """not vacuous: segments are absorbed in every case, the image is finite and differs from the one without volume records, nothing else moves"""
    spp = 2
    acc, rng, st = volume_ref.reference(oracle, name, nee, W, H, spp)
    plain, plain_rng, plain_st = volume_ref.reference(oracle, name, nee, W, H, spp, vols=None)
    _, absorbed, _ = volume_ref.per_sample(oracle, name, nee, W, H, spp)
    with capsys.disabled():
        print(f"\n{name} nee {nee}: {st.segments_absorbed} segments absorbed, {(absorbed > 0).mean():.4f} of the samples", end="")
    assert st.segments_absorbed > 0 and int(absorbed.sum()) == st.segments_absorbed
    assert np.isfinite(acc).all()
    assert (words(acc) != words(plain)).any()
    assert np.array_equal(rng, plain_rng)                                         # (a sample advances its pixel's rng by one, whatever its path did)


def test_the_roulette_sees_the_attenuated_throughput(oracle):
    """the rng after a sample is n + 1 whatever the path did, so the draws show in the ray counts: with absorption some paths end earlier"""
    _, _, st = volume_ref.reference(oracle, "room", 0, W, H, 2)
    _, _, plain_st = volume_ref.reference(oracle, "room", 0, W, H, 2, vols=None)
    assert st.extension_rays < plain_st.extension_rays


def _furnace_samples(oracle, sigma, spp=4):
    vols = volume_ref.records([sigma])
    rad, absorbed, _ = volume_ref.per_sample(oracle, "furnace", 0, W, H, spp, vols=vols)
    return rad.astype(np.float64), absorbed


def test_furnace_with_grey_absorption_keeps_the_skys_ratio_and_never_exceeds_it(oracle):
    """Glass of albedo 1 under a constant sky, grey sigma: the throughput's channels stay equal (T, Glass's spectrum 1 or albedo, the roulette's 1 / max are
    the same in all three), so a sample is RN(RN(thr * sky_c) * intensity) per channel with ONE thr <= 1, and the sky's own value s_c is the same with thr = 1
    (one rounding: 1 * sky_c is exact).  Three roundings of 2^-24 apart, to first order 6 * 2^-24 between the channels' sample_c / s_c; held to 8 * 2^-24."""
    s = model_scenes.furnace_sky_value(oracle, W, H).astype(np.float64)
    rad, absorbed = _furnace_samples(oracle, volume_ref.volumes("furnace")["sigma"][0])
    assert (absorbed > 0).any() and (absorbed == 0).any()
    assert np.all(rad <= s)                                                       # no sample exceeds the sky's value
    assert np.all((rad[absorbed == 0] == s) | (rad[absorbed == 0] == 0.0))        # untouched by the rule: the models' furnace statement, s or nothing
    lit = rad[..., 0] > 0.0
    assert (lit & (absorbed > 0)).any()
    ratio = rad[lit] / s
    assert np.all(np.abs(ratio - ratio[:, :1]) <= 8 * 2.0 ** -24 * ratio[:, :1])
    assert np.all(ratio[absorbed[lit] > 0][:, 0] < 1.0)                           # an absorbed segment darkens
    assert not rad[~lit].any()                                                    # a sample is dark in all channels or in none


def test_furnace_with_opaque_glass_is_black_wherever_a_segment_was_absorbed(oracle):
    s = model_scenes.furnace_sky_value(oracle, W, H).astype(np.float64)
    rad, absorbed = _furnace_samples(oracle, (1e30, 1e30, 1e30))
    assert (absorbed > 0).any()
    assert not rad[absorbed > 0].any()                                            # exactly 0
    assert np.all((rad[absorbed == 0] == s) | (rad[absorbed == 0] == 0.0)) and (rad[absorbed == 0] == s).any()


def _volume_glb(path):
    """one triangle and six materials: plain; glass with a volume; a volume with thicknessFactor 0; one without a distance; a colour channel of 0 (and one
    above 1); a volume on a material that is not transmissive"""
    glass = {"KHR_materials_transmission": {"transmissionFactor": 1.0}}
    materials = [{"pbrMetallicRoughness": {"baseColorFactor": [0.8, 0.7, 0.6, 1.0]}},
                 {"extensions": dict(glass, KHR_materials_volume={"thicknessFactor": 1.0, "attenuationDistance": 0.5, "attenuationColor": [0.5, 0.25, 1.0]})},
                 {"extensions": dict(glass, KHR_materials_volume={"thicknessFactor": 0.0, "attenuationDistance": 0.5, "attenuationColor": [0.5, 0.25, 1.0]})},
                 {"extensions": dict(glass, KHR_materials_volume={"thicknessFactor": 1.0, "attenuationColor": [0.5, 0.25, 1.0]})},
                 {"extensions": dict(glass, KHR_materials_volume={"thicknessFactor": 2.0, "attenuationDistance": 4.0, "attenuationColor": [0.0, 1.5, 0.1]})},
                 {"extensions": {"KHR_materials_volume": {"thicknessFactor": 1.0, "attenuationDistance": 2.0}}}]
    return scenes.write_glb(str(path), [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [0, 1, 2], materials=materials)


def test_the_loader_reads_the_volume_extension_only_when_asked(rpt, hipmod, tmp_path):
    path = _volume_glb(tmp_path / "volume.glb")
    plain, flagged = rpt.World.from_path(path), rpt.World.from_path(path, material_models=True, material_volumes=True)
    assert len(plain.material_volumes) == len(plain.materials) == 6 and not plain.material_volumes["sigma"].any()
    assert not rpt.World.from_path(path, material_models=True).material_volumes["sigma"].any()
    got = flagged.material_volumes
    assert got.dtype == hipmod.MATERIAL_VOLUME_DTYPE and not got["reserved"].any()
    f32 = np.float32
    want = np.zeros((6, 3), np.float32)
    want[1] = [f32(-np.log(0.5) / 0.5), f32(-np.log(0.25) / 0.5), 0.0]           # in double, rounded once
    want[4] = [np.finfo(np.float32).max, 0.0, f32(-np.log(0.1) / 4.0)]            # a channel of 0: FLT_MAX; 1.5 is clamped to 1
    assert np.array_equal(words(got["sigma"]), words(want)), got["sigma"]        # thicknessFactor 0, a missing distance, the default colour: zeros
    assert np.array_equal(got["sigma"][1], hipmod.absorption((0.5, 0.25, 1.0), 0.5))
    assert flagged.material_models["model"].tolist() == [0, 2, 2, 2, 2, 0]
    for field in ("per_vertex", "indices", "nodes", "materials", "light_pick"):      # the world itself does not depend on the flag
        assert getattr(plain, field).tobytes() == getattr(flagged, field).tobytes()
    a, b = tmp_path / "a.rptscene", tmp_path / "b.rptscene"
    plain.save(str(a)); flagged.save(str(b))
    assert a.read_bytes() == b.read_bytes()                                          # ... nor does the cache, which does not carry the records
    assert not rpt.World.from_cache(str(b)).material_volumes["sigma"].any()
