/*
 * lights_oracle.cpp — test-side restatement of the reference's trace_pixel (kernels/src/lib.rs:21-186) with the model switch at lib.rs:144
 * (rpt_set_material_models), the thin-lens camera at lib.rs:38-51 (rpt_set_camera_lens), the absorption rule of rpt_set_material_volumes and the punctual lights
 * of rpt_set_punctual_lights (include/rpt/rpt.h), in the oracle's own types and math.  The lights act inside sample_direct_lighting only: with n lights and
 * the effective share q, the four draws of light_pick.rs are made when there is a mesh light or a punctual light; l1 < q picks light
 * j = min(f2u32_sat((l1 / q) * n), n - 1) with pick pdf q / n, weight 1 in both NEE modes and "no triangle" as the carried light; otherwise (l1 - q) / (1 - q)
 * takes l1's place in the alias pick and the pick pdf is multiplied by 1 - q.  Nothing else differs from tests/volume_oracle/volume_oracle.cpp, whose frame
 * this is, restated: that unit and everything under oracle/ stay as they are, and this one includes oracle/rpt_oracle.cpp and tests/lens_oracle/lens_camera.h
 * textually as that one does.  With no lights it must give volume_lens_trace_cpu's words, rng and counters (tests/test_punctual_lights.py).  One more counter:
 * punctual_picks, the light samples that picked a punctual light.  Built as liblights_oracle.so with -Wl,-Bsymbolic: its copy of the oracle's exported
 * names binds to itself.
 */
#include "../../oracle/rpt_oracle.cpp"
#include "../lens_oracle/lens_camera.h"

namespace {

enum : uint32_t { MODEL_PBR = 0, MODEL_LAMBERTIAN = 1, MODEL_GLASS = 2 };
struct ModelRecord { uint32_t model; float ior; uint32_t reserved[2]; };     /* rpt_material_model */
struct VolumeRecord { float sigma[3]; uint32_t reserved; };                  /* rpt_material_volume */
enum : uint32_t { LIGHT_POINT = 0, LIGHT_SPOT = 1, LIGHT_DIRECTIONAL = 2 };
struct LightRecord { uint32_t type; float position[3], direction[3], intensity[3], angle_scale, angle_offset; uint32_t reserved[4]; };     /* rpt_punctual_light */
static_assert(sizeof(LightRecord) == 64, "rpt_punctual_light");
struct Lights { const LightRecord *records; uint32_t n; float q; bool segment; };   /* q: the effective share — 0 with no lights, 1 over a sentinel table;
                                                                                       segment: the shadow rays are walked under RPT_SHADOW_SEGMENT */

/* a BSDF behind the trait: the PBR one, or the parameters of one of the other two */
struct Surface {
    uint32_t model;
    PBR pbr;
    float ior;
};

/* the item oracle_bsdf takes: view(3) normal(3) r(3) albedo(3) ior roughness pad(2) */
inline void bsdf_item(const Surface &s, V3 view, V3 normal, V3 r, float *p) {
    p[0] = view.x; p[1] = view.y; p[2] = view.z; p[3] = normal.x; p[4] = normal.y; p[5] = normal.z; p[6] = r.x; p[7] = r.y; p[8] = r.z;
    p[9] = s.pbr.albedo.x; p[10] = s.pbr.albedo.y; p[11] = s.pbr.albedo.z; p[12] = s.ior; p[13] = s.pbr.roughness; p[14] = 0.0f; p[15] = 0.0f;
}

struct Sampled { float pdf; uint32_t lobe; V3 spectrum, direction; };

inline Sampled surface_sample(const Surface &s, V3 view, V3 normal, RngState &rng) {
    const V3 r = rng.gen_r3();                    /* every model's sample draws one gen_r3() (bsdf.rs:72, 136, 273) */
    Sampled out;
    if (s.model == MODEL_PBR) {
        const BSDFSample b = s.pbr.sample_with(view, normal, r);
        out.pdf = b.pdf; out.lobe = (uint32_t)b.sampled_lobe; out.spectrum = b.spectrum; out.direction = b.sampled_direction;
        return out;
    }
    float in[16], o[8];
    bsdf_item(s, view, normal, r, in);
    oracle_bsdf(s.model == MODEL_LAMBERTIAN ? 0 : 1, 1, in, o);
    out.pdf = o[0]; out.lobe = rptm::f2u(o[1]); out.spectrum = v3(o[2], o[3], o[4]); out.direction = v3(o[5], o[6], o[7]);
    return out;
}

/* evaluate and pdf for the diffuse reflection lobe, as sample_direct_lighting asks them (light_pick.rs:153-155); Glass never gets here */
inline void surface_evaluate_diffuse(const Surface &s, V3 view, V3 normal, V3 direction, V3 &spectrum, float &pdf) {
    if (s.model == MODEL_PBR) {
        spectrum = s.pbr.evaluate(view, normal, direction, DiffuseReflection);
        pdf = s.pbr.pdf(view, normal, direction, DiffuseReflection);
        return;
    }
    float in[16], o[8];
    bsdf_item(s, view, normal, direction, in);
    oracle_bsdf(2, 1, in, o);
    pdf = o[0]; spectrum = v3(o[2], o[3], o[4]);
}

struct ModelCounters {
    Counters walk;                      /* the oracle's own: extension_rays, shadow_rays, sky_evals, light_index_clamped, error_flags */
    uint64_t shadow_rays_zero_term = 0; /* shadow rays whose unoccluded term is zero: what the device does not queue (rpt_stats.shadow_rays_elided) */
    uint64_t segments_absorbed = 0;     /* hits at which the absorption rule multiplied the throughput by the transmittance of a sigma that is not all zero */
    uint64_t punctual_picks = 0;        /* light samples whose first draw fell below the punctual lights' share */
};

/* `.hit` of a shadow ray.  RPT_SHADOW_EXACT: the reference's any-hit walk.  RPT_SHADOW_SEGMENT (rpt.h rpt_set_shadow_mode), the restatement's own mode for
 * it: a child box is entered iff the reference's box test passes (against the 1e6 an any-hit walk carries until it returns) AND tmin <= max_t — the rule of
 * tools/anyhit_order_sim.cpp sim_any_hit_segment, restated here; the triangle test is the reference's.  `.hit` does not depend on the order in which the
 * boxes are visited (tests/test_anyhit_order.py), so this walk goes left first.  Applied to mesh and punctual shadow rays alike. */
bool shadow_ray_hits(const Scene &sc, bool segment, V3 ro, V3 rd, float max_t, Counters &cnt) {
    if (!segment) return intersect_front_to_back<false>(sc, ro, rd, max_t, cnt).hit;
    std::vector<uint32_t> work(1, 0u);
    while (!work.empty()) {
        const rpt_bvh_node &node = sc.nodes[work.back()];
        work.pop_back();
        if (node.triangle_count > 0) {
            for (uint32_t i = 0; i < node.triangle_count; ++i) {
                const rpt_triangle tri = sc.indices[node.left_or_first + i];
                float t = 0.0f;
                bool backface = false;
                if (muller_trumbore(ro, rd, xyz(sc.per_vertex[tri.v0].vertex), xyz(sc.per_vertex[tri.v1].vertex), xyz(sc.per_vertex[tri.v2].vertex), t, backface) &&
                    t > 0.001f && t < 1000000.0f && t <= max_t)
                    return true;
            }
        } else {
            const uint32_t children[2] = {node.left_or_first + 1, node.left_or_first};      /* right pushed first: left is popped first */
            for (uint32_t child : children) {
                const rpt_bvh_node &c = sc.nodes[child];
                const float tmin = intersect_aabb(xyz(c.aabb_min), xyz(c.aabb_max), ro, rd, 1000000.0f);
                if (!rptm::isinfr(tmin) && tmin <= max_t) work.push_back(child);
            }
        }
    }
    return false;
}

/* light_pick.rs:100-173 with the surface behind the trait, and the punctual lights of rpt_set_punctual_lights in front of the alias pick */
DirectLightSample sample_direct_lighting_lights(uint32_t nee_mode, const Scene &sc, V3 throughput, const Surface &surface, V3 surface_point, V3 surface_normal,
                                                V3 ray_direction, RngState &rng, const Lights &lights, ModelCounters &cnt) {
    DirectLightSample info;
    const bool sentinel = sc.light_pick[0].ratio < 0.0f;
    if (sentinel && lights.n == 0u) return info;
    V2 r = rng.gen_r2();
    float keep = 1.0f;                     /* the share of the first draw left to the table */
    if (lights.n != 0u) {
        const float q = lights.q;
        if (r.x < q) {
            cnt.punctual_picks++;
            rng.gen_r2();                  /* p1, p2: drawn, a delta light has no point to choose */
            uint32_t j = rptm::f2u32_sat((r.x / q) * (float)lights.n);
            if (j > lights.n - 1u) j = lights.n - 1u;
            const float pick_pdf = q / (float)lights.n;
            const LightRecord &l = lights.records[j];
            const V3 intensity = v3(l.intensity[0], l.intensity[1], l.intensity[2]), dir = v3(l.direction[0], l.direction[1], l.direction[2]);
            V3 light_direction, arriving;
            float max_t;
            if (l.type == LIGHT_DIRECTIONAL) {
                light_direction = -dir;
                max_t = 1e6f;
                arriving = intensity;
            } else {
                const V3 unorm = v3(l.position[0], l.position[1], l.position[2]) - surface_point;
                const float distance = length(unorm);
                light_direction = unorm / distance;
                max_t = distance - EPS * 2.0f;
                float spot = 1.0f;
                if (l.type == LIGHT_SPOT) {
                    const float a = m_min(m_max(dot(dir, -light_direction) * l.angle_scale + l.angle_offset, 0.0f), 1.0f);
                    spot = a * a;
                }
                arriving = intensity * (spot / (distance * distance));
            }
            cnt.walk.shadow_rays++;
            const V3 origin = surface_point + light_direction * EPS;
            const bool occluded = shadow_ray_hits(sc, lights.segment, origin, light_direction, max_t, cnt.walk);
            V3 unoccluded = splat3(0.0f);
            V3 bsdf_attenuation;
            float bsdf_pdf;
            surface_evaluate_diffuse(surface, -ray_direction, surface_normal, light_direction, bsdf_attenuation, bsdf_pdf);
            if (bsdf_pdf > 0.0f) unoccluded = (bsdf_attenuation * arriving) / pick_pdf;
            const V3 term = mask_nan(throughput * unoccluded);
            if (term.x == 0.0f && term.y == 0.0f && term.z == 0.0f) cnt.shadow_rays_zero_term++;
            const V3 direct = occluded ? splat3(0.0f) : unoccluded;
            info.light_pick_pdf = pick_pdf;
            info.light_triangle_index = 0xffffffffu;       /* no triangle: calculate_bsdf_mis_contribution finds no match */
            info.throughput = throughput;
            info.direct_light_contribution = throughput * direct;
            return info;
        }
        if (sentinel) {                    /* l1 == 1.0 over a share of 1: nothing to pick, nothing evaluated, nothing counted */
            rng.gen_r2();
            info.light_triangle_index = 0xffffffffu;
            return info;
        }
        keep = 1.0f - q;
        r.x = (r.x - q) / keep;
    }
    uint32_t len = (uint32_t)sc.n_light_pick;
    uint32_t idx = rptm::f2u32_sat(r.x * (float)len);
    if (idx >= len) { idx = len - 1; cnt.walk.light_index_clamped++; }
    const rpt_light_pick_entry &entry = sc.light_pick[idx];
    uint32_t light_index;
    float light_area, light_pick_pdf;
    if (r.y < entry.ratio) {
        light_index = entry.triangle_index_a; light_area = entry.triangle_area_a; light_pick_pdf = entry.triangle_pick_pdf_a;
    } else {
        light_index = entry.triangle_index_b; light_area = entry.triangle_area_b; light_pick_pdf = entry.triangle_pick_pdf_b;
    }
    light_pick_pdf = light_pick_pdf * keep;
    rpt_triangle lt = sc.indices[light_index];
    V3 va = xyz(sc.per_vertex[lt.v0].vertex), vb = xyz(sc.per_vertex[lt.v1].vertex), vc = xyz(sc.per_vertex[lt.v2].vertex);
    V3 na = xyz(sc.per_vertex[lt.v0].normal), nb = xyz(sc.per_vertex[lt.v1].normal), nc = xyz(sc.per_vertex[lt.v2].normal);
    V3 light_normal = (na + nb + nc) / 3.0f;
    V3 light_emission = xyz(sc.materials[lt.material].emissive);
    V2 r2 = rng.gen_r2();
    float r1_sqrt = m_sqrt(r2.x);
    V3 light_point = (1.0f - r1_sqrt) * va + (r1_sqrt * (1.0f - r2.y)) * vb + (r1_sqrt * r2.y) * vc;
    V3 light_direction_unorm = light_point - surface_point;
    float light_distance = length(light_direction_unorm);
    V3 light_direction = light_direction_unorm / light_distance;

    cnt.walk.shadow_rays++;
    const bool occluded = shadow_ray_hits(sc, lights.segment, surface_point + light_direction * EPS, light_direction, light_distance - EPS * 2.0f, cnt.walk);
    /* the term an unoccluded ray adds (light_pick.rs:148-160) */
    V3 unoccluded = splat3(0.0f);
    float light_pdf = calculate_light_pdf(light_area, light_distance, light_normal, light_direction);
    if (light_pdf > 0.0f) {
        V3 bsdf_attenuation;
        float bsdf_pdf;
        surface_evaluate_diffuse(surface, -ray_direction, surface_normal, light_direction, bsdf_attenuation, bsdf_pdf);
        if (bsdf_pdf > 0.0f) {
            float weight = get_weight(nee_mode, light_pdf, bsdf_pdf);
            unoccluded = (bsdf_attenuation * light_emission * weight / light_pdf) / light_pick_pdf;
        }
    }
    const V3 term = mask_nan(throughput * unoccluded);
    if (term.x == 0.0f && term.y == 0.0f && term.z == 0.0f) cnt.shadow_rays_zero_term++;
    const V3 direct = occluded ? splat3(0.0f) : unoccluded;
    info.light_area = light_area;
    info.light_normal = light_normal;
    info.light_pick_pdf = light_pick_pdf;
    info.light_emission = light_emission;
    info.light_triangle_index = light_index;
    info.throughput = throughput;
    info.direct_light_contribution = throughput * direct;
    return info;
}

/* lib.rs:21-186; lens: the camera of rpt_set_camera_lens at lib.rs:38-51, or NULL for the reference's own lines; volumes: one record per material, or NULL;
 * lights: the punctual lights with their effective share, n == 0 for none */
PixelResult trace_pixel_lights(uint32_t id_x, uint32_t id_y, const rpt_tracing_config &config, rpt_rng_state rng, const Scene &sc, const ModelRecord *models,
                               const VolumeRecord *volumes, const LensRecord *lens, const Lights &lights, ModelCounters &cnt) {
    uint32_t nee_mode = config.nee <= 2 ? config.nee : 0;
    bool nee = nee_mode != RPT_NEE_NONE;
    RngState rng_state{rng.n, rng.offset, 0, false};

    V3 ray_origin, ray_direction;
    if (lens) {
        lens_camera_ray(id_x, id_y, config, *lens, rng_state, ray_origin, ray_direction);
    } else {
        V2 jitter = rng_state.gen_r2();
        V2 suv = V2{(float)id_x, (float)id_y} + jitter;
        V2 uv = V2{suv.x / (float)config.width, 1.0f - suv.y / (float)config.height} * 2.0f - V2{1.0f, 1.0f};
        uv.y *= (float)config.height / (float)config.width;

        ray_origin = xyz(config.cam_position);
        ray_direction = normalize(v3(uv.x, uv.y, 1.0f));
        M3 euler_mat = mul(rotation_y(config.cam_rotation[1]), rotation_x(config.cam_rotation[0]));
        ray_direction = mul(euler_mat, ray_direction);
    }

    V3 throughput = splat3(1.0f);
    V3 radiance = splat3(0.0f);
    BSDFSample last_bsdf_sample;                  /* pdf, spectrum, direction of the last sample: what calculate_bsdf_mis_contribution reads */
    uint32_t last_lobe = 0u;                      /* BSDFSample::default(): DiffuseReflection */
    DirectLightSample last_light_sample;

    for (uint32_t bounce = 0; bounce < config.max_bounces; ++bounce) {
        cnt.walk.extension_rays++;
        TraceResult trace_result = intersect_front_to_back<true>(sc, ray_origin, ray_direction, 0.0f, cnt.walk);
        V3 hit = ray_origin + ray_direction * trace_result.t;

        if (!trace_result.hit) {
            cnt.walk.sky_evals++;
            if (config.has_skybox == 0) {
                radiance = radiance + throughput * sky_scatter(config.sun_direction, ray_origin, ray_direction);
            } else {
                float rotation = m_atan2(config.sun_direction[2], config.sun_direction[0]);
                V3 rotated = mul(rotation_y(rotation), ray_direction);
                float u = 0.5f + m_atan2(rotated.z, rotated.x) / (2.0f * PI_F);
                float v = 1.0f - (0.5f + m_asin(rotated.y) / PI_F);
                float intensity = config.sun_direction[3] * (1.0f / 15.0f);
                V4 s = sample_by_lod(sc.skybox, V2{u, v});
                radiance = radiance + throughput * v3(s.x, s.y, s.z) * intensity;
            }
            break;
        }

        const rpt_material_data &material = sc.materials[trace_result.triangle.material];
        if (ne_zero3(xyz(material.emissive))) {
            if (trace_result.backface) break;
            if (!nee || bounce == 0 || last_lobe != 0u) {
                radiance = radiance + mask_nan(throughput * xyz(material.emissive));
                break;
            }
            if (nee_mode == RPT_NEE_MIS && last_lobe == 0u) {
                V3 direct_contribution = calculate_bsdf_mis_contribution(trace_result, last_bsdf_sample, last_light_sample);
                radiance = radiance + mask_nan(direct_contribution);
                break;
            }
        }

        const rpt_per_vertex_data &vda = sc.per_vertex[trace_result.triangle.v0];
        const rpt_per_vertex_data &vdb = sc.per_vertex[trace_result.triangle.v1];
        const rpt_per_vertex_data &vdc = sc.per_vertex[trace_result.triangle.v2];
        V3 bary = barycentric(hit, xyz(vda.vertex), xyz(vdb.vertex), xyz(vdc.vertex));
        V3 normal = bary.x * xyz(vda.normal) + bary.y * xyz(vdb.normal) + bary.z * xyz(vdc.normal);
        V2 tuv = bary.x * V2{vda.uv0[0], vda.uv0[1]} + bary.y * V2{vdb.uv0[0], vdb.uv0[1]} + bary.z * V2{vdc.uv0[0], vdc.uv0[1]};
        {
            float cx = m_min(m_max(tuv.x, 0.0f), 1.0f), cy = m_min(m_max(tuv.y, 0.0f), 1.0f);
            if (cx != tuv.x || cy != tuv.y) tuv = V2{tuv.x - rptm::floorr(tuv.x), tuv.y - rptm::floorr(tuv.y)};
        }
        if (material.has_normal_texture != 0) {
            V2 scaled_uv = V2{material.normals[0], material.normals[1]} + tuv * V2{material.normals[2], material.normals[3]};
            V4 nm4 = sample_by_lod(sc.atlas, scaled_uv) * 2.0f - V4{1.0f, 1.0f, 1.0f, 1.0f};
            V3 tangent = bary.x * xyz(vda.tangent) + bary.y * xyz(vdb.tangent) + bary.z * xyz(vdc.tangent);
            M3 tbn = M3{tangent, cross(tangent, normal), normal};
            normal = normalize(mul(tbn, v3(nm4.x, nm4.y, nm4.z)));
        }

        /* lib.rs:144, the one line that changes */
        Surface surface;
        surface.pbr = get_pbr_bsdf(config, material, tuv, sc.atlas);
        surface.model = models ? models[trace_result.triangle.material].model : (uint32_t)MODEL_PBR;
        surface.ior = models ? models[trace_result.triangle.material].ior : 1.0f;
        /* rpt_set_material_volumes: the segment that ends here ran through this glass */
        if (volumes && surface.model == MODEL_GLASS && dot(normal, -ray_direction) < 0.0f) {
            const VolumeRecord &vr = volumes[trace_result.triangle.material];
            const V3 transmittance = v3(m_exp(-(vr.sigma[0] * trace_result.t)), m_exp(-(vr.sigma[1] * trace_result.t)), m_exp(-(vr.sigma[2] * trace_result.t)));
            throughput = throughput * transmittance;
            if (vr.sigma[0] != 0.0f || vr.sigma[1] != 0.0f || vr.sigma[2] != 0.0f) cnt.segments_absorbed++;
        }
        const Sampled bsdf_sample = surface_sample(surface, -ray_direction, normal, rng_state);
        last_bsdf_sample.pdf = bsdf_sample.pdf;
        last_bsdf_sample.spectrum = bsdf_sample.spectrum;
        last_bsdf_sample.sampled_direction = bsdf_sample.direction;
        last_lobe = bsdf_sample.lobe;

        if (nee && bsdf_sample.lobe == 0u) {
            last_light_sample = sample_direct_lighting_lights(nee_mode, sc, throughput, surface, hit, normal, ray_direction, rng_state, lights, cnt);
            radiance = radiance + mask_nan(last_light_sample.direct_light_contribution);
        }

        throughput = throughput * (bsdf_sample.spectrum / bsdf_sample.pdf);
        ray_direction = bsdf_sample.direction;
        ray_origin = hit + ray_direction * EPS;

        if (bounce > config.min_bounces) {
            float prob = max_element(throughput);
            if (rng_state.gen_r1() > prob) break;
            throughput = throughput * (1.0f / prob);
        }
    }
    if (rng_state.overflow || (lens && lens_shares_a_dimension(*lens, rng_state))) cnt.walk.error_flags |= 2u;
    PixelResult out;
    out.radiance = V4{radiance.x, radiance.y, radiance.z, 1.0f};
    out.next_n = rng.n + 1;
    out.next_offset = rng.offset;
    return out;
}


/* the effective share of rpt_set_punctual_lights: 1 over a sentinel table, else pick_share; 0 with no lights */
Lights make_lights(const Scene &sc, const LightRecord *records, uint32_t n, float pick_share, uint32_t shadow_mode) {
    if (!records || n == 0u) return Lights{nullptr, 0u, 0.0f, shadow_mode == 1u};
    return Lights{records, n, sc.light_pick[0].ratio < 0.0f ? 1.0f : pick_share, shadow_mode == 1u};
}

}  // namespace

extern "C" {

typedef struct lights_stats {
    uint64_t samples, extension_rays, shadow_rays, sky_evals, light_index_clamped;
    uint64_t shadow_rays_zero_term;      /* of shadow_rays: the term an unoccluded ray adds is zero */
    uint64_t segments_absorbed;          /* hits at which the absorption rule multiplied by a sigma that is not all zero */
    uint64_t punctual_picks;             /* light samples that picked a punctual light */
    uint32_t error_flags, threads;
} lights_stats;

/* volume_lens_trace_cpu's loop over trace_pixel_lights: n_samples passes over the rectangle rect = (x0, y0, x1, y1), rows in parallel; models, volumes, lens as
 * there; lights: n_lights records (NULL, 0: none) and the pick_share handed to rpt_set_punctual_lights; shadow_mode: 0 RPT_SHADOW_EXACT, 1 RPT_SHADOW_SEGMENT */
int lights_trace_cpu(const rpt_tracing_config *config, const oracle_scene *scene, const ModelRecord *models, const VolumeRecord *volumes, const LensRecord *lens,
                     const LightRecord *light_records, uint32_t n_lights, float pick_share, rpt_rng_state *rng, float *accum, uint32_t n_samples,
                     const uint32_t *rect, int n_threads, uint32_t shadow_mode, lights_stats *stats) {
    if (!config || !scene || !rng || !accum || !rect) return -1;
    Scene sc = make_scene(scene);
    const Lights lights = make_lights(sc, light_records, n_lights, pick_share, shadow_mode);
    const uint32_t W = config->width, H = config->height;
    const uint32_t x0 = rect[0], y0 = rect[1], x1 = rect[2] > W ? W : rect[2], y1 = rect[3] > H ? H : rect[3];
    if (n_threads <= 0) n_threads = (int)std::thread::hardware_concurrency();
    if (n_threads <= 0) n_threads = 1;
    std::vector<ModelCounters> counters((size_t)n_threads);
    for (uint32_t s = 0; s < n_samples; ++s) {
        std::atomic<uint32_t> next_row{y0};
        auto worker = [&](int tid) {
            ModelCounters &cnt = counters[(size_t)tid];
            for (;;) {
                uint32_t y = next_row.fetch_add(1);
                if (y >= y1) break;
                for (uint32_t x = x0; x < x1; ++x) {
                    size_t i = (size_t)y * W + x;
                    PixelResult r = trace_pixel_lights(x, y, *config, rng[i], sc, models, volumes, lens, lights, cnt);
                    accum[4 * i + 0] += r.radiance.x;
                    accum[4 * i + 1] += r.radiance.y;
                    accum[4 * i + 2] += r.radiance.z;
                    accum[4 * i + 3] += r.radiance.w;
                    rng[i].n = r.next_n;
                    rng[i].offset = r.next_offset;
                }
            }
        };
        if (n_threads == 1) {
            worker(0);
        } else {
            std::vector<std::thread> pool;
            for (int t = 0; t < n_threads; ++t) pool.emplace_back(worker, t);
            for (auto &t : pool) t.join();
        }
    }
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        for (const ModelCounters &c : counters) {
            stats->extension_rays += c.walk.extension_rays;
            stats->shadow_rays += c.walk.shadow_rays;
            stats->sky_evals += c.walk.sky_evals;
            stats->light_index_clamped += c.walk.light_index_clamped;
            stats->shadow_rays_zero_term += c.shadow_rays_zero_term;
            stats->segments_absorbed += c.segments_absorbed;
            stats->punctual_picks += c.punctual_picks;
            stats->error_flags |= c.walk.error_flags;
        }
        stats->samples = (uint64_t)(x1 > x0 ? x1 - x0 : 0u) * (y1 > y0 ? y1 - y0 : 0u) * n_samples;
        stats->threads = (uint32_t)n_threads;
    }
    return 0;
}

/* every pixel of the image, one sample each, in one call: radiance (H * W * 3 floats) and punctual picks (H * W words, nullable) per sample; the rng is
 * read, not advanced */
int lights_trace_samples(const rpt_tracing_config *config, const oracle_scene *scene, const ModelRecord *models, const VolumeRecord *volumes, const LensRecord *lens,
                         const LightRecord *light_records, uint32_t n_lights, float pick_share, const rpt_rng_state *rng, float *out_rgb,
                         uint32_t shadow_mode, uint64_t *punctual_picks_out) {
    if (!config || !scene || !rng || !out_rgb) return -1;
    Scene sc = make_scene(scene);
    const Lights lights = make_lights(sc, light_records, n_lights, pick_share, shadow_mode);
    int flags = 0;
    for (uint32_t y = 0; y < config->height; ++y)
        for (uint32_t x = 0; x < config->width; ++x) {
            const size_t i = (size_t)y * config->width + x;
            ModelCounters cnt;
            PixelResult r = trace_pixel_lights(x, y, *config, rng[i], sc, models, volumes, lens, lights, cnt);
            out_rgb[3 * i] = r.radiance.x; out_rgb[3 * i + 1] = r.radiance.y; out_rgb[3 * i + 2] = r.radiance.z;
            if (punctual_picks_out) punctual_picks_out[i] = cnt.punctual_picks;
            flags |= (int)cnt.walk.error_flags;
        }
    return flags;
}

/* `.hit` of n shadow rays under the restatement's walk of a shadow mode (tests/test_punctual_lights.py holds mode 1 to tools/anyhit_order_sim.cpp) */
int lights_shadow_rays(const oracle_scene *scene, size_t n, const float *origins, const float *dirs, const float *max_t, uint32_t shadow_mode, uint8_t *hit_out) {
    if (!scene || !origins || !dirs || !max_t || !hit_out) return -1;
    Scene sc = make_scene(scene);
    Counters cnt;
    for (size_t i = 0; i < n; ++i) hit_out[i] = shadow_ray_hits(sc, shadow_mode == 1u, xyz(origins + 3 * i), xyz(dirs + 3 * i), max_t[i], cnt) ? 1 : 0;
    return 0;
}

}  // extern "C"
