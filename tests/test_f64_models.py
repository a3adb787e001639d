"""The material models' bit-exact restatement (tests/models_oracle) and the oracle's BSDF functions held to an independent float64 reading of bsdf.rs
(tests/f64_models.py): sample by sample on the probe renders of tests/f64_models_probes.py, and function by function against oracle_bsdf kinds 0-3.
No GPU needed; the device is held to the restatement bit for bit (tests/test_gpu_material_models.py)."""
import numpy as np
import pytest

import f64_models
import f64_models_probes as probes
from f64_models_probes import DELTA, FLAGGED_CAP

N_ITEMS = 40000


def _items(seed, ior, roughness):
    """oracle_bsdf's items: view(3) normal(3) r(3) albedo(3) ior roughness pad(2); views from both sides of the surface"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(N_ITEMS, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    nrm = rng.normal(size=(N_ITEMS, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    items = np.zeros((N_ITEMS, 16), np.float32)
    items[:, 0:3], items[:, 3:6] = v, nrm
    items[:, 6:9] = rng.random((N_ITEMS, 3))
    items[:, 9:12] = rng.uniform(0.1, 0.95, (N_ITEMS, 3))
    items[:, 12], items[:, 13] = ior, roughness
    return items


def _rel(got, want, floor):
    return np.abs(np.asarray(got, np.float64) - want) / np.maximum(np.abs(want), floor)


def function_differences():
    """-> {function: (largest relative difference oracle_bsdf - f64_models over the compared inputs, share of the inputs left out)}.  Directions are unit
    vectors and compared against a floor of 1; pdfs and spectra against 1e-3 (a cosine that small is a grazing sample).  Glass: inputs within DELTA of the
    Fresnel decision, of `inside` or of the total-internal-reflection clamp are left out, as a sample that decides by a hair is."""
    from oracle_ffi import Oracle
    oracle = Oracle("rpt_math")
    out = {}
    for seed, (ior, roughness) in enumerate([(1.5, 0.05), (1.33, 0.9), (1.5, 0.3), (2.4, 0.001)]):
        it = _items(100 + seed, ior, roughness)
        f = it.astype(np.float64)
        view, normal, r, albedo = f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9:12]
        with np.errstate(all="ignore"):
            # kind 0: Lambertian::sample
            o, s = oracle.bsdf(0, it), f64_models.lambertian_sample(albedo, normal, r)
            d = np.concatenate([_rel(o[:, 0:1], s["pdf"][:, None], 1e-3), _rel(o[:, 2:5], s["spectrum"], 1e-3), _rel(o[:, 5:8], s["direction"], 1.0)], 1)
            assert np.all(o[:, 1].view(np.uint32) == 0)
            out.setdefault("lambertian_sample", []).append((float(d.max()), 0.0))
            # kind 2: Lambertian::evaluate and pdf, at a random unit direction
            it2 = it.copy()
            it2[:, 6:9] = it[:, 0:3][::-1]
            o = oracle.bsdf(2, it2)
            direction = it2[:, 6:9].astype(np.float64)
            d = np.concatenate([_rel(o[:, 0:1], f64_models.lambertian_pdf(normal, direction)[:, None], 1e-3),
                                _rel(o[:, 2:5], f64_models.lambertian_evaluate(albedo, normal, direction), 1e-3)], 1)
            out.setdefault("lambertian_evaluate_pdf", []).append((float(d.max()), 0.0))
            # kind 1: Glass::sample
            o, s = oracle.bsdf(1, it), f64_models.glass_sample(albedo, f[:, 12], f[:, 13], view, normal, r)
            keep = s["margin"] >= DELTA
            assert np.array_equal(o[keep, 1].view(np.uint32), s["lobe"][keep].astype(np.uint32))          # the same lobe wherever it is not decided by a hair
            d = np.concatenate([_rel(o[:, 0:1], s["pdf"][:, None], 1e-3), _rel(o[:, 2:5], s["spectrum"], 1e-3), _rel(o[:, 5:8], s["direction"], 1.0)], 1)
            out.setdefault("glass_sample", []).append((float(d[keep].max()), float(1.0 - keep.mean())))
            # kind 3: Glass::evaluate and pdf are table look-ups by lobe (bsdf.rs:115-128, 170-176): exact
            it3 = it.copy()
            it3[:, 6] = np.random.default_rng(seed).integers(0, 4, N_ITEMS)
            o = oracle.bsdf(3, it3)
            want = np.where((it3[:, 6] == 1)[:, None], 1.0, albedo)
            assert np.all(o[:, 0] == 1.0) and np.array_equal(o[:, 2:5].astype(np.float64), want)
    return {k: (max(m for m, _ in v), max(s for _, s in v)) for k, v in out.items()}


def test_the_functions_agree_with_the_oracles(capsys):
    got = function_differences()
    with capsys.disabled():
        for name, (worst, left_out) in got.items():
            print(f"\n{name}: max rel {worst:.3e}, left out {left_out:.5f}", end="")
    for name, (worst, left_out) in got.items():
        assert left_out <= FLAGGED_CAP, name
        assert worst <= probes.FUNCTION_TOL, (name, worst)


def _agrees_sample_by_sample(name, nee, lens_name=None):
    c = probes.case(name, nee, lens_name)
    share = float(c["flagged"].mean())
    d = probes.sample_differences(c)
    worst = float(np.nanmax(np.where(~c["flagged"][..., None], d, 0.0)))
    print(f"{name} nee {nee} lens {lens_name}: flagged {share:.5f}, max rel over the unflagged samples {worst:.3e}")
    assert share <= FLAGGED_CAP                               # a condition: the views were chosen so that the float64 reference alone stays under it
    assert np.isfinite(c["f64"][~c["flagged"]]).all()
    assert worst <= probes.MODELS_TOL
    assert (np.abs(c["f64"]).max(-1) > 0).any()               # (the closed room without NEE: few samples find the lamp, most compare zeros)


@pytest.mark.parametrize("name,nee", probes.CASES)
def test_the_restatement_agrees_sample_by_sample(name, nee):
    _agrees_sample_by_sample(name, nee)


@pytest.mark.parametrize("name,nee,lens_name", probes.LENS_CASES)
def test_the_restatement_with_both_switches_agrees_sample_by_sample(name, nee, lens_name):
    """the restatement with the model AND the lens (models_lens_trace_cpu) against f64_models.trace under the same lens: the same tolerance, the same cap"""
    _agrees_sample_by_sample(name, nee, lens_name)
