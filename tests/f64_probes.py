"""The probe renders of the float64 second opinion, computed once per case and shared by tests/test_f64_reference.py (CPU: oracle against f64_ref,
sample by sample) and tests/test_gpu_f64_probes.py (device against both): the oracle's per-sample radiances (SampleBank) and f64_ref's radiances and
margins.  The thresholds both modules use live here, with how they were obtained.

Re-measure with:  python tests/f64_probes.py        (prints, per case, the flagged share and the largest relative difference oracle - f64)
"""
import functools
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_ref                       # noqa: E402
import scenes                        # noqa: E402
from moments_ref import SampleBank   # noqa: E402

# A sample whose smallest decision margin (f64_ref's units) is below DELTA is flagged and not compared.  The compared quantities of a float32 path
# (random numbers against weights, barycentric coordinates, distances) carry errors of a few 1e-6 after a handful of bounces; DELTA is ten times
# that, and with some twenty decisions per path against smooth random variables the flagged share is expected at a few times twenty times DELTA, well
# under the cap of 1 %.  Measured: at most 0.19 % by decision (corner-nee1-4bounces-min2), 0.32 % with the cosine criterion below (the grazing views).
DELTA = 2e-5
FLAGGED_CAP = 0.01
# The smallest mean radiance that still shows at an 8-bit display: half a code, 0.5 / 255, through the sRGB encoding's linear toe (slope 12.92); the
# steepest tonemap operator at zero is the identity (the neutral operator's slope there is 0.99, the others are flatter).  A per-sample radiance or an
# accumulator of n samples is n times a mean, hence n times the floor.
FLOOR_MEAN = 0.5 / 255.0 / 12.92
# A sample with a specular bounce whose halfway . view (f64_ref.trace's min_cosine) is below COS_MIN is flagged as well, under the same cap: float32
# keeps a cosine to about 1e-7 absolutely, and the specular pdf divides by halfway . view, whose error near a mirror bounce is 1e-7 / cosine^2
# relatively (1e-3 at 0.01, 2e-2 at the 0.0024 of the grazing view's horizon row).  Such samples are compared no more than those that decide by a
# hair; there is no other allowance.
COS_MIN = 0.01
# |oracle - f64| / max(|f64|, floor) per sample and channel, plain, the largest over all cases' unflagged samples as printed by the command above, and
# the tolerance: eight times that.
PATH_REL_MAX = 9.32e-4          # corner-nee0-5bounces, a path into the sky's horizon; 1.3e-4 to 7.8e-4 on the other probes
PATH_TOL = 8 * PATH_REL_MAX
# A sample whose lookup in the image sky has 1 - y^2 below POLE_MIN (y the rotated direction's vertical component, f64_ref.trace's sky_y) is flagged too,
# under the same cap: the row comes from asin(y), and a float32 y in error by 1e-7 moves v by 1e-7 / sqrt(1 - y^2), which the threshold keeps below
# 1e-5.  The two caps around the poles are 5e-5 of the sphere.
POLE_MIN = 1e-4
# The textured probes, the image-sky probes and the sampler have figures and tolerances of their own (the same rule: eight times the figure), so that
# the untextured probes keep theirs.
# Textured: 1.5e-4 to 3.5e-4 on the slabs whose uvs stay in [0, 1]; where they run over [-0.8, 1.9] the uv's float32 error is 2.7 times as large, and
# times the slope of the roughness map and the normal map it is an error of the sampled specular direction and of the shading normal.  The samples that
# set the figure are single specular bounces that leave within 2e-4 .. 4e-4 of the shading normal's plane (n . direction, below the EPS at which the
# reference floors that cosine), whose geometry term is proportional to that cosine; all others of these probes are below 5e-4.
TEXTURED_REL_MAX = 2.05e-3      # tex-all-32x32-wrap-sky; 1.7e-3 on the other two wrapping slabs
TEXTURED_TOL = 8 * TEXTURED_REL_MAX
# Image sky: two arctangents, an arcsine and one lookup, and no sky march: far tighter than PATH_TOL.
IMAGE_SKY_REL_MAX = 6.19e-5     # imgsky-corner-16x8-seam-nee1 (bounced rays); 4.3e-6 to 2.8e-5 where every pixel is a lookup
IMAGE_SKY_TOL = 8 * IMAGE_SKY_REL_MAX
# The sampler, function by function (tests/test_f64_reference.py prints it): the float32 rounding of the scaled coordinate, up to 2^-18 at 3 x 65
# texels, times the difference of neighbouring texels over their value
SAMPLER_REL_MAX = 1.85e-5       # 63 x 65, float texels; 1.5e-5 at 64 x 48, below 2.1e-6 at the small extents and 2.3e-7 at 64 x 64
SAMPLER_TOL = 8 * SAMPLER_REL_MAX
GROUP_TOL = {"path": PATH_TOL, "textured": TEXTURED_TOL, "image_sky": IMAGE_SKY_TOL}


def group(name):
    return scenes.PROBE_CASES[name].get("group", "path")


def tolerance(name):
    """the tolerance of a probe's samples: that of its group"""
    return GROUP_TOL[group(name)]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(cfg, world, seeds, bank, f64 (spp, H, W, 3), margin (spp, H, W), flagged (spp, H, W))"""
    rpt = importlib.import_module("rust-path-tracer_amd")
    from oracle_ffi import Oracle
    cfg, world, skybox = scenes.probe_config(name), scenes.probe_world(name), scenes.probe_skybox(name)
    seeds = rpt.blue_noise_seeds(cfg.width, cfg.height)
    bank = SampleBank(Oracle("rpt_math"), cfg, world, seeds, skybox_f32=skybox)
    bank.need(scenes.PROBE_SPP)
    radiance, margin, min_cosine, sky_y = f64_ref.trace_image(cfg, world, seeds, 0, scenes.PROBE_SPP, skybox=skybox)
    return dict(cfg=cfg, world=world, skybox=skybox, seeds=seeds, bank=bank, f64=radiance, margin=margin, min_cosine=min_cosine, sky_y=sky_y,
                tol=tolerance(name), flagged=(margin < DELTA) | (min_cosine < COS_MIN) | (1.0 - sky_y * sky_y < POLE_MIN))


def sample_differences(c):
    """per sample and channel |oracle - f64| / max(|f64|, floor) -> (spp, H, W, 3)"""
    ora = np.stack(c["bank"].radiance[:scenes.PROBE_SPP]).astype(np.float64)
    with np.errstate(all="ignore"):
        return np.abs(ora - c["f64"]) / np.maximum(np.abs(c["f64"]), scenes.PROBE_SPP * FLOOR_MEAN)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    worst, share = {}, {}
    for name in scenes.PROBE_CASES:
        c = case(name)
        d = sample_differences(c)
        keep = ~c["flagged"]
        m = float(np.nanmax(np.where(keep[..., None], d, 0.0)))
        g = group(name)
        if m > worst.get(g, (-1.0, ""))[0]:
            worst[g] = (m, name)
        share[g] = max(share.get(g, 0.0), float(c["flagged"].mean()))
        print(f"{name:36s} flagged {c['flagged'].mean():8.5f} (by decision {(c['margin'] < DELTA).mean():.5f}, by the pole "
              f"{(1.0 - c['sky_y'] ** 2 < POLE_MIN).mean():.5f})   max rel (unflagged) {m:.3e}   max rel (all) {float(np.nanmax(d)):.3e}")
    for g, constant in (("path", "PATH_REL_MAX"), ("textured", "TEXTURED_REL_MAX"), ("image_sky", "IMAGE_SKY_REL_MAX")):
        print(f"{constant} = {worst[g][0]:.3e}   ({worst[g][1]}; largest flagged share of the group {share[g]:.5f})")
