"""The bit-exact restatement of punctual lights (tests/lights_oracle) held to an independent float64 reading of the rule in rpt.h (tests/f64_lights.py),
sample by sample on its probe renders, under tests/f64_probes.py's rule.  No GPU needed; the device is held to the restatement bit for bit
(tests/test_gpu_punctual_lights.py)."""
import numpy as np
import pytest

import f64_lights
from f64_probes import FLAGGED_CAP


@pytest.mark.parametrize("name,nee", f64_lights.CASES)
def test_the_restatement_agrees_sample_by_sample(name, nee, capsys):
    c = f64_lights.case(name, nee)
    share = float(c["flagged"].mean())
    d = f64_lights.sample_differences(c)
    worst = float(np.nanmax(np.where(~c["flagged"][..., None], d, 0.0)))
    picked = c["picks"] > 0
    with capsys.disabled():
        print(f"\n{name} nee {nee}: flagged {share:.5f}, a punctual pick in {picked.mean():.4f} of the samples, max rel over the unflagged samples {worst:.3e}", end="")
    assert share <= FLAGGED_CAP                               # a condition: the lights sit well clear of every surface, so the float64 reading alone stays under it
    assert np.isfinite(c["f64"][~c["flagged"]]).all()
    assert worst <= f64_lights.LIGHTS_TOL
    keep = ~c["flagged"]
    assert picked.any() and np.array_equal(c["picks"][keep].astype(np.int64), c["picks_f64"][keep])      # both readings pick a punctual light in the same samples
    assert (np.abs(c["f64"][picked & keep]).max(-1) > 0).any()                # ... and compare more than zeros there


def test_the_float64_reading_without_lights_is_f64_models(rpt):
    """f64_lights.trace restates f64_models.trace's loop: with no lights the two agree to the last bit of float64"""
    import f64_models
    import model_scenes
    W, H = 16, 12
    world, rec, skybox, _ = model_scenes.scene("room")
    for nee in (0, 1):
        cfg, seeds = model_scenes.config("room", nee, W, H), rpt.blue_noise_seeds(W, H)
        want = f64_models.trace_image(cfg, world, rec, seeds, 0, 2, skybox=skybox)
        got = f64_lights.trace_image(cfg, world, rec, None, 0.5, seeds, 0, 2, skybox=skybox)
        for a, b in zip(got[:4], want):
            assert np.array_equal(a, b, equal_nan=True)
        assert not got[4].any()
