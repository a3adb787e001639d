"""A float64 second opinion on punctual lights (include/rpt/rpt.h rpt_set_punctual_lights): tests/f64_models.py's tracer — trace_pixel's loop with the model
switch, in numpy float64 — with the rule as rpt.h states it, written from that text and not from the C++: the share q of the first light draw, the pick
j = min(floor((l1 / q) n), n - 1) with pdf q / n, the term intensity * spot / d^2 (or the irradiance) times the surface's diffuse evaluate over the pick pdf with
weight 1, "no triangle" as the carried light; otherwise (l1 - q) / (1 - q) in l1's place and the pick pdf times 1 - q.  Everything else is f64_models' and
f64_ref's, imported; the loop is restated for the one call.  The decisions the rule adds: l1 against q (margin |l1 - q|), the light index (the distance of
(l1 / q) n to the next integer, with more than one light), and the shadow ray's (f64_ref.intersect_any's).  The cone's clamps and the horizon test are
continuous in the term and need none.

The probe renders hold the bit-exact restatement (tests/lights_oracle) to this reading sample by sample under tests/f64_probes.py's rule: a sample whose
smallest decision margin is below DELTA (or whose specular cosine or sky pole is) is flagged and not compared, the flagged share is capped at FLAGGED_CAP per
case, and the tolerance is eight times the largest relative difference measured over the unflagged samples.  Scenes room, open and textured with the lights of
tests/lights_ref.py — one of each type, well clear of every surface — and a share of 0.5, at 32 x 24, scenes.PROBE_SPP samples per pixel, MIS and direct-only.

Re-measure with:  python tests/f64_lights.py      (prints, per case, the flagged share, the share of samples with a punctual pick and the largest relative difference)
"""
import functools
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f64_ref                       # noqa: E402
import lights_ref                    # noqa: E402
import model_scenes                  # noqa: E402
import scenes                        # noqa: E402
from f64_models import MODEL_GLASS, MODEL_LAMBERTIAN, glass_sample, intersect_any, intersect_nearest, lambertian_evaluate, lambertian_pdf, lambertian_sample      # noqa: E402
from f64_probes import COS_MIN, DELTA, FLAGGED_CAP, FLOOR_MEAN, POLE_MIN      # noqa: E402,F401
from f64_ref import DIFFUSE, EPS, INF, col, dot, normalize      # noqa: E402

SIZE = (32, 24)
CASES = [(name, nee) for name in ("room", "open", "textured") for nee in (1, 2)]
# |restatement - f64| / max(|f64|, floor) per sample and channel, the largest over the unflagged samples of all cases as the command above prints it, and
# the tolerance: eight times that
# Measured on the CPU: textured 1.714e-3 (MIS and direct-only alike: the texture lookup's float32 uv under a glossy bounce, the sample that sets
# MODELS_REL_MAX of f64_models_probes and VOLUMES_REL_MAX of f64_volumes too); open 2.92e-4 (the sky march behind a refraction); room 1.63e-4.  Flagged shares:
# room 0.13 %, open 0.07 %, textured 0.03 %.  Samples with a punctual pick: room 74 %, open 54 %, textured 12 %; both readings pick a punctual light in the
# same unflagged samples.
LIGHTS_REL_MAX = 1.714e-3       # textured, nee 1 and nee 2
LIGHTS_TOL = 8 * LIGHTS_REL_MAX


def direct_lighting(mis, sc, rng, mask, throughput, bsdf, lambert, point, normal, ray_direction, clamp, lights, q):
    """sample_direct_lighting (light_pick.rs:100-173) with the surface behind the trait and the rule of rpt_set_punctual_lights in front of the alias pick;
    lights: records (type, position, direction, intensity, angle_scale, angle_offset) or None, q: the effective share"""
    L = sc.light
    has_mesh = L["ratio"][0] >= 0.0
    n_lights = 0 if lights is None else len(lights)
    N = len(point)
    r = rng.r2(mask)
    p = rng.r2(mask)
    l1, l2 = r[:, 0], r[:, 1]
    punctual = (l1 < q) if n_lights else np.zeros(N, bool)
    margin = np.abs(l1 - q) if (n_lights and 0.0 < q < 1.0) else np.full(N, INF)
    view = -ray_direction
    diffuse = np.full(N, DIFFUSE)

    def surface(direction):
        attenuation = np.where(col(lambert), lambertian_evaluate(bsdf["albedo"], normal, direction),
                               f64_ref.pbr_evaluate(view, normal, direction, diffuse, bsdf["albedo"], bsdf["roughness"], bsdf["metallic"], clamp))
        return attenuation, np.where(lambert, lambertian_pdf(normal, direction), f64_ref.pbr_pdf(view, normal, direction, diffuse, bsdf["roughness"]))

    out = dict(area=np.zeros(N), normal=np.zeros((N, 3)), pick_pdf=np.ones(N), emission=np.zeros((N, 3)), triangle=np.full(N, -1, np.int64),
               throughput=throughput, contribution=np.zeros((N, 3)), margin=margin)
    if n_lights:
        x = (l1 / q) * n_lights
        j = np.clip(np.floor(x), 0, n_lights - 1).astype(np.int64)
        if n_lights > 1:
            m_index = np.where(x >= n_lights, INF, np.minimum(x - np.floor(x), np.floor(x) + 1.0 - x))
            out["margin"] = np.where(punctual, np.minimum(out["margin"], m_index), out["margin"])
        kind = np.asarray(lights["type"], np.int64)[j]
        position, aim = np.asarray(lights["position"], np.float64)[j], np.asarray(lights["direction"], np.float64)[j]
        intensity = np.asarray(lights["intensity"], np.float64)[j]
        scale, offset = np.asarray(lights["angle_scale"], np.float64)[j], np.asarray(lights["angle_offset"], np.float64)[j]
        v = position - point
        d = np.sqrt(dot(v, v))
        toward = v / col(d)
        a = np.clip(dot(aim, -toward) * scale + offset, 0.0, 1.0)
        spot = np.where(kind == lights_ref.SPOT, a * a, 1.0)
        arriving = intensity * col(spot / (d * d))
        directional = kind == lights_ref.DIRECTIONAL
        toward = np.where(col(directional), -aim, toward)
        max_t = np.where(directional, 1e6, d - EPS * 2.0)
        arriving = np.where(col(directional), intensity, arriving)
        pick_pdf = q / n_lights
        occluded, m_shadow = intersect_any(sc, point + toward * EPS, toward, max_t)
        attenuation, bp = surface(toward)
        direct = attenuation * arriving / pick_pdf                      # weight 1 in both NEE modes
        unoccluded = np.where(col(bp > 0.0), throughput * direct, 0.0)
        m_shadow = np.where(np.abs(unoccluded).max(-1) > f64_ref.SHADOW_MATTERS, m_shadow, INF)
        direct = np.where(col(~occluded & (bp > 0.0)), direct, 0.0)
        out["contribution"] = np.where(col(punctual), throughput * direct, out["contribution"])
        out["margin"] = np.where(punctual, np.minimum(out["margin"], m_shadow), out["margin"])
    if has_mesh:
        keep = 1.0 - q
        u = (l1 - q) / keep
        n_entries = len(L["ratio"])
        x = u * float(n_entries)
        entry = np.clip(np.where(np.isfinite(x), x, 0.0).astype(np.int64), 0, n_entries - 1)
        m_pick = np.where(x >= n_entries, 0.0, np.minimum(x - np.floor(x), np.floor(x) + 1.0 - x)) if n_entries > 1 else np.where(x >= n_entries, 0.0, INF)
        first = l2 < L["ratio"][entry]
        same = L["triangle_index_a"][entry] == L["triangle_index_b"][entry]
        m_pick = np.minimum(m_pick, np.where(same, INF, np.abs(l2 - L["ratio"][entry])))
        tri = np.where(first, L["triangle_index_a"][entry], L["triangle_index_b"][entry])
        area = np.where(first, L["triangle_area_a"][entry], L["triangle_area_b"][entry])
        pick_pdf = np.where(first, L["triangle_pick_pdf_a"][entry], L["triangle_pick_pdf_b"][entry]) * keep
        idx = sc.tri[tri]
        l_normal = (sc.normal[idx[:, 0]] + sc.normal[idx[:, 1]] + sc.normal[idx[:, 2]]) / 3.0
        emission = sc.emissive[sc.material[tri]]
        s = np.sqrt(p[:, 0])
        l_point = col(1.0 - s) * sc.a[tri] + col(s * (1.0 - p[:, 1])) * sc.b[tri] + col(s * p[:, 1]) * sc.c[tri]
        to_light = l_point - point
        distance = np.sqrt(dot(to_light, to_light))
        direction = to_light / col(distance)
        occluded, m_shadow = intersect_any(sc, point + direction * EPS, direction, distance - EPS * 2.0)
        lp = f64_ref.light_pdf(area, distance, l_normal, direction)
        attenuation, bp = surface(direction)
        weight = f64_ref.power_heuristic(lp, bp) if mis else 1.0
        direct = attenuation * emission * col(weight) / col(lp) / col(pick_pdf)
        unoccluded = np.where(col((lp > 0.0) & (bp > 0.0)), throughput * direct, 0.0)
        m_shadow = np.where(np.abs(unoccluded).max(-1) > f64_ref.SHADOW_MATTERS, m_shadow, INF)
        direct = np.where(col(~occluded & (lp > 0.0) & (bp > 0.0)), direct, 0.0)
        mesh = ~punctual
        for key, value in (("area", area), ("pick_pdf", pick_pdf), ("triangle", tri)):
            out[key] = np.where(mesh, value, out[key])
        for key, value in (("normal", l_normal), ("emission", emission), ("contribution", throughput * direct)):
            out[key] = np.where(col(mesh), value, out[key])
        out["margin"] = np.where(mesh, np.minimum(out["margin"], np.minimum(m_pick, m_shadow)), out["margin"])
    out["punctual"] = punctual
    return out


def trace(cfg, world, models, lights, share, px, py, n, offset, skybox=None):
    """f64_models.trace with the lights -> (radiance (N, 3), margin, min_cosine, sky_y, picks (N,) = the light samples that picked a punctual light)"""
    sc = world if isinstance(world, f64_ref.Scene) else f64_ref.Scene(world, skybox)
    model_of, ior_of = np.asarray(models["model"], np.int64), np.asarray(models["ior"], np.float64)
    n_lights = 0 if lights is None else len(lights)
    has_mesh = sc.light["ratio"][0] >= 0.0
    q = 0.0 if n_lights == 0 else (float(np.float32(share)) if has_mesh else 1.0)
    N = len(px)
    nee_mode = cfg.nee if cfg.nee <= 2 else 0
    nee, mis = nee_mode != 0, nee_mode == 1
    clamp = (float(cfg.specular_weight_clamp[0]), float(cfg.specular_weight_clamp[1]))
    rng = f64_ref.Rng(n, offset)
    every = np.ones(N, bool)
    with np.errstate(all="ignore"):
        jitter = rng.r2(every)
        origin, direction = f64_ref.camera_rays(cfg, np.asarray(px, np.float64), np.asarray(py, np.float64), jitter)
        throughput, radiance, margin, alive, min_cosine = np.ones((N, 3)), np.zeros((N, 3)), np.full(N, INF), every.copy(), np.full(N, INF)
        sky_y = np.zeros(N)
        picks = np.zeros(N, np.int64)
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
            if glass.any():
                g = glass_sample(albedo, ior_of[mat], roughness, view, normal, r3)
                decide(g.pop("margin"), glass)
                s = f64_ref._update(s, g, glass)
            last_bsdf = f64_ref._update(last_bsdf, s, alive)

            # rpt.h, rpt_set_punctual_lights: the four draws are made exactly when NEE runs and there is a mesh light or a punctual light
            lit = alive & nee & (s["lobe"] == DIFFUSE)
            if lit.any() and (has_mesh or n_lights):
                ls = direct_lighting(mis, sc, rng, lit, throughput, bsdf, lit & lambert, point, normal, direction, clamp, lights, q)
                decide(ls.pop("margin"), lit)
                picks = picks + (lit & ls.pop("punctual"))
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
    return radiance, margin, min_cosine, sky_y, picks


def trace_image(cfg, world, models, lights, share, seeds, first_sample, n_samples, skybox=None):
    """-> (radiance (n_samples, H, W, 3), margin, min_cosine, sky_y, picks (n_samples, H, W) each)"""
    W, H = cfg.width, cfg.height
    sc = f64_ref.Scene(world, skybox)
    py, px = np.divmod(np.arange(W * H), W)
    out = [], [], [], [], []
    for k in range(first_sample, first_sample + n_samples):
        r, m, c, y, a = trace(cfg, sc, models, lights, share, px, py, seeds["n"].astype(np.uint64) + np.uint64(k), seeds["offset"])
        for o, a in zip(out, (r.reshape(H, W, 3), m.reshape(H, W), c.reshape(H, W), y.reshape(H, W), a.reshape(H, W))):
            o.append(a)
    return tuple(np.stack(o) for o in out)


@functools.lru_cache(maxsize=None)
def case(name, nee):
    """-> dict(cfg, restated (spp, H, W, 3) f32 per-sample radiances, f64 (spp, H, W, 3), margin, flagged, picks (the restatement's), picks_f64 (spp, H, W))"""
    rpt = importlib.import_module("rust-path-tracer_amd")
    from oracle_ffi import Oracle
    W, H = SIZE
    world, rec, skybox, _ = model_scenes.scene(name)
    lts = lights_ref.lights(name)
    cfg = model_scenes.config(name, nee, W, H)
    seeds = rpt.blue_noise_seeds(W, H)
    restated, picks, _starts = lights_ref.per_sample(Oracle("rpt_math"), name, nee, W, H, scenes.PROBE_SPP)
    radiance, margin, min_cosine, sky_y, picks_f64 = trace_image(cfg, world, rec, lts, lights_ref.SHARE, seeds, 0, scenes.PROBE_SPP, skybox=skybox)
    return dict(cfg=cfg, restated=restated, f64=radiance, margin=margin, min_cosine=min_cosine, sky_y=sky_y, picks=picks, picks_f64=picks_f64,
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
        print(f"{name:10s} nee {nee}   flagged {c['flagged'].mean():8.5f} (by decision {(c['margin'] < DELTA).mean():.5f})   punctual {(c['picks'] > 0).mean():.4f}   "
              f"max rel (unflagged) {m:.3e}   max rel (all) {float(np.nanmax(d)):.3e}   picks agree {np.array_equal(c['picks'][keep].astype(np.int64), c['picks_f64'][keep])}")
    print(f"LIGHTS_REL_MAX = {worst[0]:.3e}   {worst[1]}")
