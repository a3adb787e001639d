"""The production kernels (k_shade.h, k_sky_generate.h, the shadow stage) on the probe scenes of tests/scenes.py, held to two references at once:

  * the CPU oracle, bit for bit, accumulators and ray counts: new scenes and material edges (roughness 0 and 1e-3, metallic 1, a zero albedo channel,
    an open clamp, grazing views, a single-sided lamp seen from both sides, roulette; every texture flag alone and together on a power-of-two and on a
    24 x 20 atlas, wrapped and negative uvs, tangents that are neither unit nor orthogonal, 16 x 8 and 7 x 5 image skies with the seam in view) for the suite's usual kind of check, which keeps device = oracle
    closed on them;
  * tests/f64_ref.py, the independent float64 restatement, within the tolerance measured between it and the oracle (tests/f64_probes.py): for every
    pixel none of whose samples is flagged, the accumulator is within the sum of its samples' tolerances of the float64 sum.

The oracle's share of the same comparison, sample by sample and without a GPU, is tests/test_f64_reference.py::test_oracle_probe_samples_against_f64.
The device BSDF has no function-level hook (the sampling code lives inside the shade stage); these probes are its share.
Re-measure the figures with   python tests/f64_probes.py
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_probes    # noqa: E402
import scenes        # noqa: E402

pytestmark = pytest.mark.gpu
SPP = scenes.PROBE_SPP


@pytest.mark.parametrize("name", list(scenes.PROBE_CASES))
def test_device_probe_equals_oracle_and_agrees_with_f64(renderer, name):
    c = f64_probes.case(name)
    cfg, bank = c["cfg"], c["bank"]
    renderer.upload_scene(c["world"], skybox_f32=c["skybox"])
    renderer.set_config(cfg)
    renderer.reset(c["seeds"])
    renderer.render(SPP)
    acc, samples = renderer.read_accum()
    st = renderer.stats()
    assert samples == SPP

    # device == oracle, bit for bit
    want, counts = bank.accum(SPP), bank.ray_counts(SPP)
    for k, v in counts.items():
        assert st[k] == v, (k, st[k], v)
    assert np.array_equal(acc.view(np.uint32), want.view(np.uint32)), "accumulators differ bitwise from the oracle"

    # device against float64: per pixel, over the pixels none of whose samples is flagged
    flagged = c["flagged"]
    share = float(flagged.mean())
    assert share <= f64_probes.FLAGGED_CAP
    clean = ~flagged.any(0)
    f64 = c["f64"]
    total = f64.sum(0)
    # a sample's tolerance: its probe's (PATH_TOL, TEXTURED_TOL or IMAGE_SKY_TOL) of max(|radiance|, floor), the floor that of one sample of SPP; the
    # float32 additions of the accumulator add SPP roundings of the sum
    per_sample = c["tol"] * np.maximum(np.abs(f64), SPP * f64_probes.FLOOR_MEAN)
    tol = per_sample.sum(0) + SPP * 2.0 ** -24 * np.abs(total)
    diff = np.abs(acc[..., :3].astype(np.float64) - total)
    worst = float(np.max(np.where(clean[..., None], diff / np.maximum(np.abs(total), SPP * f64_probes.FLOOR_MEAN), 0.0)))
    print(f"{name}: flagged samples {share:.5f}, pixels compared {int(clean.sum())} of {clean.size}, largest relative difference of an accumulator {worst:.3e}")
    assert clean.mean() > 0.9
    assert np.isfinite(acc).all() and np.isfinite(total).all()                # flagged or not: nothing is NaN or infinite where float64 is finite
    assert np.all((diff <= tol) | ~clean[..., None]), "a device accumulator is outside the float64 restatement's tolerance"
