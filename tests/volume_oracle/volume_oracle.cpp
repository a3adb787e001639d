/*
 * volume_oracle.cpp — test-side restatement of the reference's trace_pixel (kernels/src/lib.rs:21-186) with the model switch at lib.rs:144
 * (rpt_set_material_models), the thin-lens camera at lib.rs:38-51 (rpt_set_camera_lens) and the absorption rule of rpt_set_material_volumes
 * (include/rpt/rpt.h): at the hit (t, triangle) of an extension ray, after the emission branch has not ended the path, iff the material's model is Glass
 * and dot(normal, view) < 0 with the normal handed to Glass::sample,
 *     T_c = exp(-(sigma_c * t))      throughput = throughput * T      before      throughput = throughput * (spectrum / pdf)
 * in the oracle's own types and math (m_exp: rptm::expr, or libm's expf in a libm build).  Nothing else differs from tests/models_oracle/models_oracle.cpp,
 * whose frame this is, restated: that unit and everything under oracle/ stay as they are, and this one includes oracle/rpt_oracle.cpp and
 * tests/lens_oracle/lens_camera.h textually as that one does.  With no volume records, and with all-zero ones, it must give models_lens_trace_cpu's words,
 * rng and counters (tests/test_material_volumes.py).  One more counter: segments_absorbed, the hits at which the rule multiplied by a sigma that is not all
 * zero.  Built as libvolume_oracle.so with -Wl,-Bsymbolic: its copy of the oracle's exported names binds to itself.
 */
#include "../../oracle/rpt_oracle.cpp"
#include "../lens_oracle/lens_camera.h"

namespace {

enum : uint32_t { MODEL_PBR = 0, MODEL_LAMBERTIAN = 1, MODEL_GLASS = 2 };
struct ModelRecord { uint32_t model; float ior; uint32_t reserved[2]; };     /* rpt_material_model */
struct VolumeRecord { float sigma[3]; uint32_t reserved; };                  /* rpt_material_volume */

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
};

/* light_pick.rs:100-173 with the surface behind the trait */
DirectLightSample sample_direct_lighting_models(uint32_t nee_mode, const Scene &sc, V3 throughput, const Surface &surface, V3 surface_point, V3 surface_normal,
                                                V3 ray_direction, RngState &rng, ModelCounters &cnt) {
    DirectLightSample info;
    if (sc.light_pick[0].ratio < 0.0f) return info;   /* sentinel */
    V2 r = rng.gen_r2();
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
    TraceResult light_trace = intersect_front_to_back<false>(sc, surface_point + light_direction * EPS, light_direction, light_distance - EPS * 2.0f, cnt.walk);
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
    const V3 direct = light_trace.hit ? splat3(0.0f) : unoccluded;
    info.light_area = light_area;
    info.light_normal = light_normal;
    info.light_pick_pdf = light_pick_pdf;
    info.light_emission = light_emission;
    info.light_triangle_index = light_index;
    info.throughput = throughput;
    info.direct_light_contribution = throughput * direct;
    return info;
}

/* lib.rs:21-186; lens: the camera of rpt_set_camera_lens at lib.rs:38-51, or NULL for the reference's own lines; volumes: one record per material, or NULL */
PixelResult trace_pixel_volumes(uint32_t id_x, uint32_t id_y, const rpt_tracing_config &config, rpt_rng_state rng, const Scene &sc, const ModelRecord *models,
                                const VolumeRecord *volumes, const LensRecord *lens, ModelCounters &cnt) {
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
            last_light_sample = sample_direct_lighting_models(nee_mode, sc, throughput, surface, hit, normal, ray_direction, rng_state, cnt);
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

}  // namespace

extern "C" {

typedef struct volume_stats {
    uint64_t samples, extension_rays, shadow_rays, sky_evals, light_index_clamped;
    uint64_t shadow_rays_zero_term;      /* of shadow_rays: the term an unoccluded ray adds is zero */
    uint64_t segments_absorbed;          /* hits at which the rule multiplied by a sigma that is not all zero */
    uint32_t error_flags, threads;
} volume_stats;

/* oracle_trace_cpu's loop (src/trace.rs:273-308) over trace_pixel_models: n_samples passes over the rectangle rect = (x0, y0, x1, y1), rows in parallel;
 * models: one record per material, or NULL for "every material is PBR"; volumes: one record per material, or NULL for none; lens: a record, or NULL for the
 * reference's camera */
int volume_lens_trace_cpu(const rpt_tracing_config *config, const oracle_scene *scene, const ModelRecord *models, const VolumeRecord *volumes, const LensRecord *lens,
                          rpt_rng_state *rng, float *accum, uint32_t n_samples, const uint32_t *rect, int n_threads, volume_stats *stats) {
    if (!config || !scene || !rng || !accum || !rect) return -1;
    Scene sc = make_scene(scene);
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
                    PixelResult r = trace_pixel_volumes(x, y, *config, rng[i], sc, models, volumes, lens, cnt);
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
            stats->error_flags |= c.walk.error_flags;
        }
        stats->samples = (uint64_t)(x1 > x0 ? x1 - x0 : 0u) * (y1 > y0 ? y1 - y0 : 0u) * n_samples;
        stats->threads = (uint32_t)n_threads;
    }
    return 0;
}

/* one pixel-sample: its radiance (the sample-by-sample comparisons) and, when asked, how many of its segments were absorbed */
int volume_lens_trace_pixel(const rpt_tracing_config *config, const oracle_scene *scene, const ModelRecord *models, const VolumeRecord *volumes, const LensRecord *lens,
                            uint32_t x, uint32_t y, rpt_rng_state rng, float *out_rgb, uint64_t *segments_absorbed_out) {
    Scene sc = make_scene(scene);
    ModelCounters cnt;
    PixelResult r = trace_pixel_volumes(x, y, *config, rng, sc, models, volumes, lens, cnt);
    out_rgb[0] = r.radiance.x; out_rgb[1] = r.radiance.y; out_rgb[2] = r.radiance.z;
    if (segments_absorbed_out) *segments_absorbed_out = cnt.segments_absorbed;
    return (int)cnt.walk.error_flags;
}

/* every pixel of the image, one sample each, in one call: radiance (H * W * 3 floats) and absorbed segments (H * W words, nullable) per sample; the rng is
 * read, not advanced */
int volume_lens_trace_samples(const rpt_tracing_config *config, const oracle_scene *scene, const ModelRecord *models, const VolumeRecord *volumes,
                              const LensRecord *lens, const rpt_rng_state *rng, float *out_rgb, uint64_t *segments_absorbed_out) {
    if (!config || !scene || !rng || !out_rgb) return -1;
    Scene sc = make_scene(scene);
    int flags = 0;
    for (uint32_t y = 0; y < config->height; ++y)
        for (uint32_t x = 0; x < config->width; ++x) {
            const size_t i = (size_t)y * config->width + x;
            ModelCounters cnt;
            PixelResult r = trace_pixel_volumes(x, y, *config, rng[i], sc, models, volumes, lens, cnt);
            out_rgb[3 * i] = r.radiance.x; out_rgb[3 * i + 1] = r.radiance.y; out_rgb[3 * i + 2] = r.radiance.z;
            if (segments_absorbed_out) segments_absorbed_out[i] = cnt.segments_absorbed;
            flags |= (int)cnt.walk.error_flags;
        }
    return flags;
}

}  // extern "C"
