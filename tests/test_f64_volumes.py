"""The bit-exact restatement of absorbing glass (tests/volume_oracle) held to an independent float64 reading of the rule in rpt.h (tests/f64_volumes.py),
sample by sample on its probe renders, under tests/f64_probes.py's rule.  No GPU needed; the device is held to the restatement bit for bit
(tests/test_gpu_material_volumes.py)."""
import numpy as np
import pytest

import f64_volumes
from f64_probes import FLAGGED_CAP


@pytest.mark.parametrize("name,nee", f64_volumes.CASES)
def test_the_restatement_agrees_sample_by_sample(name, nee, capsys):
    c = f64_volumes.case(name, nee)
    share = float(c["flagged"].mean())
    d = f64_volumes.sample_differences(c)
    worst = float(np.nanmax(np.where(~c["flagged"][..., None], d, 0.0)))
    absorbed = c["absorbed"] > 0
    with capsys.disabled():
        print(f"\n{name} nee {nee}: flagged {share:.5f}, absorbed {absorbed.mean():.4f} of the samples, max rel over the unflagged samples {worst:.3e}", end="")
    assert share <= FLAGGED_CAP                               # a condition: sigma and view were chosen so that the float64 reading alone stays under it
    assert np.isfinite(c["f64"][~c["flagged"]]).all()
    assert worst <= f64_volumes.VOLUMES_TOL
    keep = ~c["flagged"]
    assert absorbed.any() and np.array_equal(c["absorbed"][keep].astype(np.int64), c["absorbed_f64"][keep])      # both readings attenuate the same segments
    assert (np.abs(c["f64"][absorbed & keep]).max(-1) > 0).any()              # ... and compare more than zeros there


def test_the_float64_reading_without_records_is_f64_models(rpt, hipmod):
    """f64_volumes.trace restates f64_models.trace's loop: with no volume records, and with all-zero ones, the two agree to the last bit of float64"""
    import f64_models
    import model_scenes
    W, H = 16, 12
    world, rec, skybox, _ = model_scenes.scene("room")
    cfg, seeds = model_scenes.config("room", 1, W, H), rpt.blue_noise_seeds(W, H)
    want = f64_models.trace_image(cfg, world, rec, seeds, 0, 2, skybox=skybox)
    for vols in (None, hipmod.material_volumes(np.zeros((len(rec), 3)))):      # (the binding's own all-zero records)
        got = f64_volumes.trace_image(cfg, world, rec, vols, seeds, 0, 2, skybox=skybox)
        for a, b in zip(got[:4], want):
            assert np.array_equal(a, b, equal_nan=True)
        assert not got[4].any()
