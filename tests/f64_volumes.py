"""A float64 second opinion on absorbing glass (include/rpt/rpt.h rpt_set_material_volumes): tests/f64_models.py's tracer — trace_pixel's loop with the model
switch, in numpy float64 — with the rule as rpt.h states it, T = exp(-sigma t) in float64, written from that text and not from the C++.  Everything else is
f64_models' and f64_ref's, imported; the loop is restated for the one multiplication.  The decision the rule adds, `inside`, is Glass::sample's own
(bsdf.rs:131): its margin |normal . view| is already one of f64_models.glass_sample's.

The probe renders hold the bit-exact restatement (tests/volume_oracle) to this reading sample by sample under tests/f64_probes.py's rule: a sample whose
smallest decision margin is below DELTA (or whose specular cosine or sky pole is) is flagged and not compared, the flagged share is capped at FLAGGED_CAP per
case, and the tolerance is eight times the largest relative difference measured over the unflagged samples.  Scenes room, open and textured
(tests/volume_ref.py: tests/model_scenes.py's with volume records) at 32 x 24, scenes.PROBE_SPP samples per pixel, nee 0 and MIS.

Re-measure with:  python tests/f64_volumes.py      (prints, per case, the flagged share, the share of samples absorbed and the largest relative difference)
"""
import functools
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_ref                       # noqa: E402
import model_scenes                  # noqa: E402
import scenes                        # noqa: E402
import volume_ref                    # noqa: E402
from f64_models import MODEL_GLASS, MODEL_LAMBERTIAN, _direct_lighting, glass_sample, intersect_nearest, lambertian_sample      # noqa: E402
from f64_probes import COS_MIN, DELTA, FLAGGED_CAP, FLOOR_MEAN, POLE_MIN      # noqa: E402,F401
from f64_ref import DIFFUSE, EPS, INF, col, dot, normalize      # noqa: E402

SIZE = (32, 24)
CASES = [(name, nee) for name in ("room", "open", "textured") for nee in (0, 1)]
# |restatement - f64| / max(|f64|, floor) per sample and channel, the largest over the unflagged samples of all cases as the command above prints it, and
# the tolerance: eight times that
# Measured on the CPU: textured 1.723e-3 (nee 0 and MIS alike: the texture lookup's float32 uv under a glossy bounce that sets MODELS_REL_MAX of
# f64_models_probes too, 1.714e-3 there, here behind a transmittance); open 3.07e-4 (the sky march behind a refraction); room 1.09e-5 without NEE,
# 5.37e-4 with MIS.  Flagged shares: room 0.13 % / 0.18 %, open 0.03 %, textured 0 / 0.02 %.  Samples with an absorbed segment: room 42 % / 37 %,
# open 9.7 %, textured 1.7 %.
VOLUMES_REL_MAX = 1.723e-3      # textured, nee 0 and nee 1
VOLUMES_TOL = 8 * VOLUMES_REL_MAX


def trace(cfg, world, models, volumes, px, py, n, offset, skybox=None, lens=None):
    """f64_models.trace with the absorption rule: models = records with fields model, ior, volumes = records with field sigma (or None), one per material
    -> (radiance (N, 3), margin, min_cosine, sky_y, absorbed (N,) = the segments the rule attenuated by a sigma that is not all zero).
    lens: (tan_half_fov, aperture_radius, focus_distance) of rpt_set_camera_lens, or None for the reference's camera; the ray is then the float64 reading
    of csrc/k_lens.h's formulas in tests/lens_ref.py rays_f64, whose only f32 inputs are the record and the LDS draws (the jitter's two, which the rng
    below draws as well, and entries 0 and 31)"""
    sc = world if isinstance(world, f64_ref.Scene) else f64_ref.Scene(world, skybox)
    model_of, ior_of = np.asarray(models["model"], np.int64), np.asarray(models["ior"], np.float64)
    sigma_of = np.zeros((len(model_of), 3)) if volumes is None else np.asarray(volumes["sigma"], np.float64).reshape(-1, 3)
    N = len(px)
    nee_mode = cfg.nee if cfg.nee <= 2 else 0
    nee, mis = nee_mode != 0, nee_mode == 1
    clamp = (float(cfg.specular_weight_clamp[0]), float(cfg.specular_weight_clamp[1]))
    rng = f64_ref.Rng(n, offset)
    every = np.ones(N, bool)
    with np.errstate(all="ignore"):
        jitter = rng.r2(every)
        if lens is None:
            origin, direction = f64_ref.camera_rays(cfg, np.asarray(px, np.float64), np.asarray(py, np.float64), jitter)
        else:
            import lens_ref
            keys = ((np.asarray(n, np.uint64) + np.asarray(offset, np.uint64)) & np.uint64(0xFFFFFFFF)) * np.ones(N, np.uint64)
            xy = np.asarray(px, np.uint64) | (np.asarray(py, np.uint64) << np.uint64(16))
            origin, direction = lens_ref.rays_f64(cfg, lens, xy, keys)[:2]
        throughput, radiance, margin, alive, min_cosine = np.ones((N, 3)), np.zeros((N, 3)), np.full(N, INF), every.copy(), np.full(N, INF)
        sky_y = np.zeros(N)
        absorbed = np.zeros(N, np.int64)
        last_bsdf = dict(pdf=np.zeros(N), lobe=np.zeros(N, np.int64), spectrum=np.zeros((N, 3)), direction=np.zeros((N, 3)))
        last_light = dict(area=np.zeros(N), normal=np.zeros((N, 3)), pick_pdf=np.zeros(N), emission=np.zeros((N, 3)), triangle=np.zeros(N, np.int64),
                          throughput=np.zeros((N, 3)))

        def decide(m, mask):
            nonlocal margin
            margin = np.where(mask, np.minimum(margin, m), margin)

        for bounce in range(cfg.max_bounces):
            if not alive.any():
                break
            hit, t, tri, backface, m_hit = intersect_nearest(sc, origin, direction)
            decide(m_hit, alive)
            point = origin + direction * col(t)
            miss = alive & ~hit
            if miss.any() and cfg.has_skybox == 0:
                radiance = radiance + np.where(col(miss), throughput * f64_ref.sky(cfg.sun_direction, origin, direction), 0.0)
            elif miss.any():
                rgb, y = f64_ref.image_sky(cfg, sc.skybox, direction)
                radiance = radiance + np.where(col(miss), throughput * rgb, 0.0)
                sky_y = np.where(miss, y, sky_y)
            alive = alive & hit

            mat = sc.material[tri]
            emitter = alive & sc.is_emitter[mat]
            front = emitter & ~backface
            direct_hit = front & (not nee or bounce == 0 or (last_bsdf["lobe"] != DIFFUSE))
            radiance = radiance + np.where(col(direct_hit), f64_ref.mask_nan(throughput * sc.emissive[mat]), 0.0)
            by_mis = front & ~direct_hit & mis
            radiance = radiance + np.where(col(by_mis), f64_ref.mask_nan(f64_ref.bsdf_mis_contribution(t, tri, last_bsdf, last_light)), 0.0)
            alive = alive & ~(emitter & backface) & ~direct_hit & ~by_mis

            idx = sc.tri[tri]
            bary = f64_ref.barycentric(point, sc.a[tri], sc.b[tri], sc.c[tri])
            normal = bary[:, 0:1] * sc.normal[idx[:, 0]] + bary[:, 1:2] * sc.normal[idx[:, 1]] + bary[:, 2:3] * sc.normal[idx[:, 2]]
            uv = bary[:, 0:1] * sc.uv[idx[:, 0]] + bary[:, 1:2] * sc.uv[idx[:, 1]] + bary[:, 2:3] * sc.uv[idx[:, 2]]
            outside = ((uv < 0.0) | (uv > 1.0)).any(1)
            uv = np.where(col(outside), uv - np.floor(uv), uv)
            textured = alive & sc.textured[mat]
            if textured.any():
                decide(np.abs(uv - np.rint(uv)).min(1), textured)
                if sc.flag["normals"].any():
                    normal_map = f64_ref._lookup(sc, "normals", mat, uv) * 2.0 - 1.0
                    tangent = bary[:, 0:1] * sc.tangent[idx[:, 0]] + bary[:, 1:2] * sc.tangent[idx[:, 1]] + bary[:, 2:3] * sc.tangent[idx[:, 2]]
                    mapped = normalize(tangent * normal_map[:, 0:1] + f64_ref.cross(tangent, normal) * normal_map[:, 1:2] + normal * normal_map[:, 2:3])
                    normal = np.where(col(sc.flag["normals"][mat]), mapped, normal)
            albedo, roughness, metallic = sc.rect["albedo"][mat][:, :3], sc.rect["roughness"][mat][:, 0], sc.rect["metallic"][mat][:, 0]
            if textured.any():
                if sc.flag["albedo"].any():
                    albedo = np.where(col(sc.flag["albedo"][mat]), f64_ref._lookup(sc, "albedo", mat, uv)[:, :3], albedo)
                if sc.flag["roughness"].any():
                    roughness = np.where(sc.flag["roughness"][mat], f64_ref._lookup(sc, "roughness", mat, uv)[:, 0], roughness)
                if sc.flag["metallic"].any():
                    metallic = np.where(sc.flag["metallic"][mat], f64_ref._lookup(sc, "metallic", mat, uv)[:, 0], metallic)
            roughness, metallic = f64_ref.pbr_guards(roughness, metallic)
            bsdf = dict(albedo=albedo, roughness=roughness, metallic=metallic)

            # lib.rs:144: the BSDF behind the trait
            model = model_of[mat]
            lambert, glass = alive & (model == MODEL_LAMBERTIAN), alive & (model == MODEL_GLASS)
            pbr = alive & ~lambert & ~glass
            r3 = rng.r3(alive)
            view = -direction
            s = f64_ref.pbr_sample(view, normal, r3, albedo, roughness, metallic, clamp)
            decide(s.pop("margin"), pbr)
            min_cosine = np.where(pbr, np.minimum(min_cosine, s.pop("min_cosine")), min_cosine)
            if lambert.any():
                s = f64_ref._update(s, lambertian_sample(albedo, normal, r3), lambert)
            # rpt.h, rpt_set_material_volumes: at the hit of an extension ray, after the emission branch has not ended the path, iff the model is Glass and
            # dot(normal, view) < 0 with the normal handed to Glass::sample: T = exp(-sigma t), throughput = throughput * T, before the sample's own factor.
            # (|normal . view|, the margin of `inside`, is one of glass_sample's below)
            inside = glass & (dot(normal, view) < 0.0)
            if inside.any():
                sigma = sigma_of[mat]
                throughput = np.where(col(inside), throughput * np.exp(-sigma * col(t)), throughput)
                absorbed = absorbed + (inside & (sigma != 0.0).any(1))
            if glass.any():
                g = glass_sample(albedo, ior_of[mat], roughness, view, normal, r3)
                decide(g.pop("margin"), glass)
                s = f64_ref._update(s, g, glass)
            last_bsdf = f64_ref._update(last_bsdf, s, alive)

            lit = alive & nee & (s["lobe"] == DIFFUSE)
            if lit.any() and sc.light["ratio"][0] >= 0.0:
                ls = _direct_lighting(mis, sc, rng, lit, throughput, bsdf, lit & lambert, point, normal, direction, clamp)
                decide(ls.pop("margin"), lit)
                radiance = radiance + np.where(col(lit), f64_ref.mask_nan(ls.pop("contribution")), 0.0)
                last_light = f64_ref._update(last_light, ls, lit)

            throughput = np.where(col(alive), throughput * (s["spectrum"] / col(s["pdf"])), throughput)
            direction = np.where(col(alive), s["direction"], direction)
            origin = np.where(col(alive), point + direction * EPS, origin)

            if bounce > cfg.min_bounces:
                prob = throughput.max(1)
                r = rng.r1(alive)
                decide(np.abs(r - prob), alive)
                alive = alive & ~(r > prob)
                throughput = np.where(col(alive), throughput * col(1.0 / prob), throughput)
    return radiance, margin, min_cosine, sky_y, absorbed


def trace_image(cfg, world, models, volumes, seeds, first_sample, n_samples, skybox=None, lens=None):
    """f64_models.trace_image with the volume records -> (radiance (n_samples, H, W, 3), margin, min_cosine, sky_y, absorbed (n_samples, H, W) each)"""
    W, H = cfg.width, cfg.height
    sc = f64_ref.Scene(world, skybox)
    py, px = np.divmod(np.arange(W * H), W)
    out = [], [], [], [], []
    for k in range(first_sample, first_sample + n_samples):
        r, m, c, y, a = trace(cfg, sc, models, volumes, px, py, seeds["n"].astype(np.uint64) + np.uint64(k), seeds["offset"], lens=lens)
        for o, a in zip(out, (r.reshape(H, W, 3), m.reshape(H, W), c.reshape(H, W), y.reshape(H, W), a.reshape(H, W))):
            o.append(a)
    return tuple(np.stack(o) for o in out)


@functools.lru_cache(maxsize=None)
def case(name, nee):
    """-> dict(cfg, restated (spp, H, W, 3) f32 per-sample radiances, f64 (spp, H, W, 3), margin, flagged, absorbed (the restatement's), absorbed_f64 (spp, H, W))"""
    rpt = importlib.import_module("rust-path-tracer_amd")
    from oracle_ffi import Oracle
    W, H = SIZE
    world, rec, skybox, _ = model_scenes.scene(name)
    vols = volume_ref.volumes(name)
    cfg = model_scenes.config(name, nee, W, H)
    seeds = rpt.blue_noise_seeds(W, H)
    restated, absorbed, _starts = volume_ref.per_sample(Oracle("rpt_math"), name, nee, W, H, scenes.PROBE_SPP)
    radiance, margin, min_cosine, sky_y, absorbed_f64 = trace_image(cfg, world, rec, vols, seeds, 0, scenes.PROBE_SPP, skybox=skybox)
    return dict(cfg=cfg, restated=restated, f64=radiance, margin=margin, min_cosine=min_cosine, sky_y=sky_y, absorbed=absorbed, absorbed_f64=absorbed_f64,
                flagged=(margin < DELTA) | (min_cosine < COS_MIN) | (1.0 - sky_y * sky_y < POLE_MIN))


def sample_differences(c):
    with np.errstate(all="ignore"):
        return np.abs(c["restated"].astype(np.float64) - c["f64"]) / np.maximum(np.abs(c["f64"]), scenes.PROBE_SPP * FLOOR_MEAN)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    worst = (-1.0, None)
    for name, nee in CASES:
        c = case(name, nee)
        d = sample_differences(c)
        keep = ~c["flagged"]
        m = float(np.nanmax(np.where(keep[..., None], d, 0.0)))
        worst = max(worst, (m, (name, nee)))
        print(f"{name:10s} nee {nee}   flagged {c['flagged'].mean():8.5f} (by decision {(c['margin'] < DELTA).mean():.5f})   absorbed {(c['absorbed'] > 0).mean():.4f}   "
              f"max rel (unflagged) {m:.3e}   max rel (all) {float(np.nanmax(d)):.3e}")
    print(f"VOLUMES_REL_MAX = {worst[0]:.3e}   {worst[1]}")
