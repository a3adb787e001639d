/*
 * lens_oracle.cpp — test-side restatement of the reference's trace_pixel (kernels/src/lib.rs:21-186) with the camera of lib.rs:38-51 replaced by the thin
 * lens of rpt_set_camera_lens (include/rpt/rpt.h): lens_camera_ray of lens_camera.h beside this file, which tests/models_oracle shares,
 * and everything from lib.rs:53 on is the oracle's text.  The oracle's trace_pixel hard-wires the pinhole and stays as it is: this unit includes
 * oracle/rpt_oracle.cpp textually to reach its internals (the walk, the sky, the sampler, the rng, the BSDF, sample_direct_lighting).
 * With the default record {1, 0, 1, 0} it must give oracle_trace_cpu's words and counters (tests/test_camera_lens.py).
 * Built as oracle/liblens_oracle.so with -Wl,-Bsymbolic: its copy of the oracle's exported names binds to itself.
 */
#include "../../oracle/rpt_oracle.cpp"

#include "lens_camera.h"

namespace {

/* lib.rs:21-186 with lens_camera_ray at lib.rs:38-51 */
PixelResult trace_pixel_lens(uint32_t id_x, uint32_t id_y, const rpt_tracing_config &config, const LensRecord &lens, rpt_rng_state rng, const Scene &sc, Counters &cnt) {
    uint32_t nee_mode = config.nee <= 2 ? config.nee : 0;
    bool nee = nee_mode != RPT_NEE_NONE;
    RngState rng_state{rng.n, rng.offset, 0, false};

    V3 ray_origin, ray_direction;
    lens_camera_ray(id_x, id_y, config, lens, rng_state, ray_origin, ray_direction);

    V3 throughput = splat3(1.0f);
    V3 radiance = splat3(0.0f);
    BSDFSample last_bsdf_sample;
    DirectLightSample last_light_sample;

    for (uint32_t bounce = 0; bounce < config.max_bounces; ++bounce) {
        cnt.extension_rays++;
        TraceResult trace_result = intersect_front_to_back<true>(sc, ray_origin, ray_direction, 0.0f, cnt);
        V3 hit = ray_origin + ray_direction * trace_result.t;

        if (!trace_result.hit) {
            cnt.sky_evals++;
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
            if (!nee || bounce == 0 || last_bsdf_sample.sampled_lobe != DiffuseReflection) {
                radiance = radiance + mask_nan(throughput * xyz(material.emissive));
                break;
            }
            if (nee_mode == RPT_NEE_MIS && last_bsdf_sample.sampled_lobe == DiffuseReflection) {
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

        PBR bsdf = get_pbr_bsdf(config, material, tuv, sc.atlas);
        BSDFSample bsdf_sample = bsdf.sample(-ray_direction, normal, rng_state);
        last_bsdf_sample = bsdf_sample;

        if (nee && bsdf_sample.sampled_lobe == DiffuseReflection) {
            last_light_sample = sample_direct_lighting(nee_mode, sc, throughput, bsdf, hit, normal, ray_direction, rng_state, cnt);
            radiance = radiance + mask_nan(last_light_sample.direct_light_contribution);
        }

        throughput = throughput * (bsdf_sample.spectrum / bsdf_sample.pdf);
        ray_direction = bsdf_sample.sampled_direction;
        ray_origin = hit + ray_direction * EPS;

        if (bounce > config.min_bounces) {
            float prob = max_element(throughput);
            if (rng_state.gen_r1() > prob) break;
            throughput = throughput * (1.0f / prob);
        }
    }
    if (rng_state.overflow || lens_shares_a_dimension(lens, rng_state)) cnt.error_flags |= 2u;
    PixelResult out;
    out.radiance = V4{radiance.x, radiance.y, radiance.z, 1.0f};
    out.next_n = rng.n + 1;
    out.next_offset = rng.offset;
    return out;
}

const LensRecord LENS_DEFAULT = {1.0f, 0.0f, 1.0f, 0u};

}  // namespace

extern "C" {

typedef struct lens_stats {
    uint64_t samples, extension_rays, shadow_rays, sky_evals, light_index_clamped;
    uint64_t shadow_rays_zero_term;      /* of shadow_rays: the term an unoccluded ray adds is zero (the device does not queue them: rpt_stats.shadow_rays_elided) */
    uint32_t error_flags, threads;
} lens_stats;

/* oracle_trace_cpu's loop (src/trace.rs:273-308) over trace_pixel_lens: n_samples passes over the rectangle rect = (x0, y0, x1, y1), rows in parallel;
 * lens NULL = the default record */
int lens_trace_cpu(const rpt_tracing_config *config, const oracle_scene *scene, const LensRecord *lens, rpt_rng_state *rng, float *accum, uint32_t n_samples,
                   const uint32_t *rect, int n_threads, lens_stats *stats) {
    if (!config || !scene || !rng || !accum || !rect) return -1;
    const LensRecord l = lens ? *lens : LENS_DEFAULT;
    Scene sc = make_scene(scene);
    const uint32_t W = config->width, H = config->height;
    const uint32_t x0 = rect[0], y0 = rect[1], x1 = rect[2] > W ? W : rect[2], y1 = rect[3] > H ? H : rect[3];
    if (n_threads <= 0) n_threads = (int)std::thread::hardware_concurrency();
    if (n_threads <= 0) n_threads = 1;
    std::vector<Counters> counters((size_t)n_threads);
    struct Dead { uint64_t v[4] = {0, 0, 0, 0}; };
    std::vector<Dead> dead((size_t)n_threads);       /* the oracle's hook: [shadow rays, of them with a zero term, of those occluded, all occluded] */
    for (uint32_t s = 0; s < n_samples; ++s) {
        std::atomic<uint32_t> next_row{y0};
        auto worker = [&](int tid) {
            Counters &cnt = counters[(size_t)tid];
            g_dead_shadow_rays = dead[(size_t)tid].v;
            for (;;) {
                uint32_t y = next_row.fetch_add(1);
                if (y >= y1) break;
                for (uint32_t x = x0; x < x1; ++x) {
                    size_t i = (size_t)y * W + x;
                    PixelResult r = trace_pixel_lens(x, y, *config, l, rng[i], sc, cnt);
                    accum[4 * i + 0] += r.radiance.x;
                    accum[4 * i + 1] += r.radiance.y;
                    accum[4 * i + 2] += r.radiance.z;
                    accum[4 * i + 3] += r.radiance.w;
                    rng[i].n = r.next_n;
                    rng[i].offset = r.next_offset;
                }
            }
            g_dead_shadow_rays = nullptr;
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
        for (const Counters &c : counters) {
            stats->extension_rays += c.extension_rays;
            stats->shadow_rays += c.shadow_rays;
            stats->sky_evals += c.sky_evals;
            stats->light_index_clamped += c.light_index_clamped;
            stats->error_flags |= c.error_flags;
        }
        for (const Dead &d : dead) stats->shadow_rays_zero_term += d.v[1];
        stats->samples = (uint64_t)(x1 > x0 ? x1 - x0 : 0u) * (y1 > y0 ? y1 - y0 : 0u) * n_samples;
        stats->threads = (uint32_t)n_threads;
    }
    return 0;
}

/* one pixel-sample: its radiance */
int lens_trace_pixel(const rpt_tracing_config *config, const oracle_scene *scene, const LensRecord *lens, uint32_t x, uint32_t y, rpt_rng_state rng, float *out_rgb) {
    if (!config || !scene || !out_rgb) return -1;
    Scene sc = make_scene(scene);
    Counters cnt;
    PixelResult r = trace_pixel_lens(x, y, *config, lens ? *lens : LENS_DEFAULT, rng, sc, cnt);
    out_rgb[0] = r.radiance.x; out_rgb[1] = r.radiance.y; out_rgb[2] = r.radiance.z;
    return (int)cnt.error_flags;
}

/* rays only: the camera rays of n (pixel x | y << 16, key) pairs — the key taken as the sample's n with offset 0 */
int lens_rays(const rpt_tracing_config *config, const LensRecord *lens, const uint32_t *pixels_xy, const uint32_t *keys, size_t n, float *origins_out, float *dirs_out) {
    if (!config || (n && (!pixels_xy || !keys || !origins_out || !dirs_out))) return -1;
    const LensRecord l = lens ? *lens : LENS_DEFAULT;
    for (size_t i = 0; i < n; ++i) {
        RngState rng_state{keys[i], 0u, 0, false};
        V3 o, d;
        lens_camera_ray(pixels_xy[i] & 0xffffu, pixels_xy[i] >> 16, *config, l, rng_state, o, d);
        origins_out[3 * i] = o.x; origins_out[3 * i + 1] = o.y; origins_out[3 * i + 2] = o.z;
        dirs_out[3 * i] = d.x; dirs_out[3 * i + 1] = d.y; dirs_out[3 * i + 2] = d.z;
    }
    return 0;
}

}  // extern "C"
