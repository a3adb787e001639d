"""A float64 second opinion on the material models (include/rpt/rpt.h rpt_set_material_models): Lambertian (kernels/src/bsdf.rs:46-105) and Glass
(bsdf.rs:107-176, util.rs:117-142, 233-236) read once more from the reference's text into numpy float64, and trace_pixel's loop (lib.rs:21-186) with the
model switch at lib.rs:144.  The bit-exact restatement (tests/models_oracle) and the kernel (csrc/k_bsdf_extra.h) come from ONE reading of bsdf.rs; this is
a second one.  Everything that is not about the models — the triangle test, sky, sampler, rng, the PBR BSDF — is f64_ref's, imported; the loop and the light sample
are restated for the switch, and the walk's margin leaves out triangles the ray is clear of (_clear_of).

Decision margins, beside the ones f64_ref.trace records: |r.z - fresnel| (reflect or refract), |normal . view| (`inside`), |1 + eta (c^2 - 1)| at the
clamp of total internal reflection."""
import numpy as np

import f64_ref
from f64_ref import DIFFUSE, EPS, INF, PI, col, create_cartesian, dot, normalize, vec

MODEL_PBR, MODEL_LAMBERTIAN, MODEL_GLASS = 0, 1, 2
SPECULAR_REFLECTION, SPECULAR_TRANSMISSION = 1, 3          # LobeType (bsdf.rs:11-16)


def _to_world(s, up, nt, nb):
    return normalize(s[..., 0:1] * nb + s[..., 1:2] * up + s[..., 2:3] * nt)


def lambertian_sample(albedo, normal, r):
    """bsdf.rs:71-92 -> dict(pdf, lobe, spectrum, direction)"""
    up, nt, nb = create_cartesian(normal)
    direction = _to_world(f64_ref.cosine_sample_hemisphere(r[..., 0], r[..., 1]), up, nt, nb)
    cos_theta = np.maximum(dot(normal, direction), 0.0)
    return dict(pdf=cos_theta / PI, lobe=np.full(cos_theta.shape, DIFFUSE), spectrum=albedo / PI * col(cos_theta), direction=direction)


def lambertian_evaluate(albedo, normal, direction):
    """bsdf.rs:59-69"""
    return albedo / PI * col(np.maximum(dot(normal, direction), 0.0))


def lambertian_pdf(normal, direction):
    """bsdf.rs:94-104"""
    return np.maximum(dot(normal, direction), 0.0) / PI


def glass_sample(albedo, ior, roughness, view, normal, r):
    """bsdf.rs:130-168 -> dict(pdf, lobe, spectrum, direction, margin)"""
    ndv = dot(normal, view)
    inside = ndv < 0.0
    n = np.where(col(inside), -normal, normal)
    in_ior, out_ior = np.where(inside, ior, 1.0), np.where(inside, 1.0, ior)
    # sample_ggx_microsurface_normal (util.rs:117-142)
    a_g = roughness * roughness
    theta = np.arctan(a_g * np.sqrt(r[..., 0]) / np.sqrt(1.0 - r[..., 0]))
    phi = 2.0 * PI * r[..., 1]
    m_local = vec(np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi))
    up, nt, nb = create_cartesian(n)
    m = _to_world(m_local, up, nt, nb)
    fresnel = f64_ref.fresnel_schlick_scalar(in_ior, out_ior, np.maximum(dot(m, view), 0.0))
    reflects = r[..., 2] <= fresnel
    reflected = normalize(2.0 * col(np.abs(dot(view, m))) * m - view)
    eta = in_ior / out_ior
    c = dot(view, m)
    under_root = 1.0 + eta * (c * c - 1.0)
    sign = np.where(np.signbit(dot(view, n)), -1.0, 1.0)                # f32::signum
    refracted = normalize(col(eta * c - sign * np.sqrt(np.maximum(under_root, 0.0))) * m - col(eta) * view)
    margin = np.minimum(np.abs(r[..., 2] - fresnel), np.abs(ndv))
    margin = np.minimum(margin, np.where(reflects, INF, np.abs(under_root)))
    return dict(pdf=np.ones(ndv.shape), lobe=np.where(reflects, SPECULAR_REFLECTION, SPECULAR_TRANSMISSION),
                spectrum=np.where(col(reflects), 1.0, albedo), direction=np.where(col(reflects), reflected, refracted), margin=margin)


def _clear_of(sc, ro, rd):
    """(n_rays, n_triangles): the ray's LINE passes the triangle's bounding sphere (about its centroid) by more than a thousandth of its radius.  Such a
    triangle is missed whatever its determinant test says — a hit lies inside the triangle — so that test's margin is no decision of the sample.
    f64_ref's own rule counts a failed determinant test of ANY triangle (its other slacks are not finite there); with the eight triangles of its probes
    that is nothing, with a 320-triangle sphere tested by every ray of an 8-bounce path it alone flagged 1.4 % of the room's samples, each for a triangle
    nowhere near the ray."""
    centre = (sc.a + sc.b + sc.c) / 3.0
    radius = np.sqrt(np.maximum(np.maximum(dot(sc.a - centre, sc.a - centre), dot(sc.b - centre, sc.b - centre)), dot(sc.c - centre, sc.c - centre)))
    to = centre[None] - ro[:, None, :]
    along = dot(to, rd[:, None, :])
    apart = np.sqrt(np.maximum(dot(to, to) - along * along / dot(rd, rd)[:, None], 0.0))
    return apart > 1.001 * radius[None]


def intersect_nearest(sc, ro, rd):
    """f64_ref.intersect_nearest, the margins of triangles the ray is clear of left out"""
    with np.errstate(all="ignore"):
        hit, t, backface, margin = f64_ref._moller_trumbore(sc, ro, rd)
        margin = np.where(~hit & _clear_of(sc, ro, rd), INF, margin)
        tt = np.where(hit, t, INF)
        order = np.argsort(tt, axis=1, kind="stable")
        rows = np.arange(len(ro))
        first = order[:, 0]
        t1 = tt[rows, first]
        t2 = tt[rows, order[:, 1]] if tt.shape[1] > 1 else np.full(len(ro), INF)
        any_hit = np.isfinite(t1)
        gap = np.where(np.isfinite(t2), (t2 - t1) / np.maximum(1.0, t1), INF)
        return any_hit, np.where(any_hit, t1, f64_ref.T_FAR), first, backface[rows, first] & any_hit, np.minimum(margin.min(1), gap)


def intersect_any(sc, ro, rd, max_t):
    """f64_ref.intersect_any, likewise"""
    with np.errstate(all="ignore"):
        hit, t, _, margin = f64_ref._moller_trumbore(sc, ro, rd)
        margin = np.where(~hit & _clear_of(sc, ro, rd), INF, margin)
        within = t <= max_t[:, None]
        m_max = np.abs(max_t[:, None] - t) / np.maximum(1.0, np.abs(t))
        margin = np.where(hit, np.minimum(margin, m_max), margin)
        return (hit & within).any(1), margin.min(1)


def _direct_lighting(mis, sc, rng, mask, throughput, bsdf, lambert, point, normal, ray_direction, clamp):
    """f64_ref.sample_direct_lighting (light_pick.rs:100-173) with the surface behind the trait at light_pick.rs:153-155 — PBR's or Lambertian's evaluate
    and pdf for the diffuse reflection — and the shadow ray's margin by the rule above"""
    L = sc.light
    n_entries = len(L["ratio"])
    r = rng.r2(mask)
    x = r[:, 0] * float(n_entries)
    entry = np.minimum(x.astype(np.int64), n_entries - 1)
    m_pick = np.where(x >= n_entries, 0.0, np.minimum(x - np.floor(x), np.floor(x) + 1.0 - x)) if n_entries > 1 else np.where(x >= n_entries, 0.0, INF)
    first = r[:, 1] < L["ratio"][entry]
    same = L["triangle_index_a"][entry] == L["triangle_index_b"][entry]
    m_pick = np.minimum(m_pick, np.where(same, INF, np.abs(r[:, 1] - L["ratio"][entry])))
    tri = np.where(first, L["triangle_index_a"][entry], L["triangle_index_b"][entry])
    area = np.where(first, L["triangle_area_a"][entry], L["triangle_area_b"][entry])
    pick_pdf = np.where(first, L["triangle_pick_pdf_a"][entry], L["triangle_pick_pdf_b"][entry])
    idx = sc.tri[tri]
    l_normal = (sc.normal[idx[:, 0]] + sc.normal[idx[:, 1]] + sc.normal[idx[:, 2]]) / 3.0
    emission = sc.emissive[sc.material[tri]]
    r = rng.r2(mask)
    s = np.sqrt(r[:, 0])
    l_point = col(1.0 - s) * sc.a[tri] + col(s * (1.0 - r[:, 1])) * sc.b[tri] + col(s * r[:, 1]) * sc.c[tri]
    to_light = l_point - point
    distance = np.sqrt(dot(to_light, to_light))
    direction = to_light / col(distance)
    occluded, m_shadow = intersect_any(sc, point + direction * EPS, direction, distance - EPS * 2.0)
    lp = f64_ref.light_pdf(area, distance, l_normal, direction)
    view = -ray_direction
    diffuse = np.full(len(point), DIFFUSE)
    attenuation = np.where(col(lambert), lambertian_evaluate(bsdf["albedo"], normal, direction),
                           f64_ref.pbr_evaluate(view, normal, direction, diffuse, bsdf["albedo"], bsdf["roughness"], bsdf["metallic"], clamp))
    bp = np.where(lambert, lambertian_pdf(normal, direction), f64_ref.pbr_pdf(view, normal, direction, diffuse, bsdf["roughness"]))
    weight = f64_ref.power_heuristic(lp, bp) if mis else 1.0
    direct = attenuation * emission * col(weight) / col(lp) / col(pick_pdf)
    unoccluded = np.where(col((lp > 0.0) & (bp > 0.0)), throughput * direct, 0.0)
    m_shadow = np.where(np.abs(unoccluded).max(-1) > f64_ref.SHADOW_MATTERS, m_shadow, INF)
    direct = np.where(col(~occluded & (lp > 0.0) & (bp > 0.0)), direct, 0.0)
    return dict(area=area, normal=l_normal, pick_pdf=pick_pdf, emission=emission, triangle=tri, throughput=throughput,
                contribution=throughput * direct, margin=np.minimum(m_pick, m_shadow))


def trace(cfg, world, models, px, py, n, offset, skybox=None, lens=None):
    """f64_ref.trace with the model switch: models = records with fields model, ior, one per material -> (radiance (N, 3), margin, min_cosine, sky_y).
    lens: (tan_half_fov, aperture_radius, focus_distance) of rpt_set_camera_lens, or None for the reference's camera; the ray is then the float64 reading
    of csrc/k_lens.h's formulas in tests/lens_ref.py rays_f64, whose only f32 inputs are the record and the LDS draws (the jitter's two, which the rng
    below draws as well, and entries 0 and 31)"""
    sc = world if isinstance(world, f64_ref.Scene) else f64_ref.Scene(world, skybox)
    model_of, ior_of = np.asarray(models["model"], np.int64), np.asarray(models["ior"], np.float64)
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
    return radiance, margin, min_cosine, sky_y


def trace_image(cfg, world, models, seeds, first_sample, n_samples, skybox=None, lens=None):
    """f64_ref.trace_image with the records -> (radiance (n_samples, H, W, 3), margin, min_cosine, sky_y (n_samples, H, W) each)"""
    W, H = cfg.width, cfg.height
    sc = f64_ref.Scene(world, skybox)
    py, px = np.divmod(np.arange(W * H), W)
    out = [], [], [], []
    for k in range(first_sample, first_sample + n_samples):
        r, m, c, y = trace(cfg, sc, models, px, py, seeds["n"].astype(np.uint64) + np.uint64(k), seeds["offset"], lens=lens)
        for o, a in zip(out, (r.reshape(H, W, 3), m.reshape(H, W), c.reshape(H, W), y.reshape(H, W))):
            o.append(a)
    return tuple(np.stack(o) for o in out)
