/*
 * k_denoise.h — the denoise step of the reference's render loop (src/trace.rs:205-213, the "Denoise" checkbox of src/app.rs:245-249) on the device:
 * first-hit guide buffers + an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the mean image, with albedo demodulation.
 * Opt-in, after the accumulator: nothing of the wavefront pipeline is touched.  Deterministic, no atomics; the per-pixel arithmetic is ONE RPT_HD
 * function (dn_filter_pixel) that the device kernel and the host build (rpt_debug_denoise_host) both call — f32, no contraction, IEEE division,
 * rptm::expr — so the two agree bit for bit, and tests/denoise_ref.py restates it in numpy with the same operation order (DESIGN.md "Denoiser").
 *
 * Guides (per pixel of the WHOLE image, whatever the context's partition), from the primary ray through the pixel centre:
 *   first hit                    kind   albedo                          normal                                   depth   position
 *   none                         0      (1,1,1)                         (0,0,0)                                  1e6     ro + rd * 1e6
 *   emissive triangle, any face  2      (1,1,1)                         shading normal (lib.rs:125-141), unit    t       ro + rd * t
 *   any other triangle           1      get_pbr_bsdf's (bsdf.rs:355-361) the same                                t       ro + rd * t
 * packed for the filter as two float4 per pixel: (normal | depth) and (position | kind bits); the albedo is its own image (read by the pre-pass
 * and by the last pass only).  A tap of a pass reads 48 bytes: colour + the two guide records.
 *
 * A second filter beside the first (rpt_denoise_variance): dn_filter_pixel_var, the same pass with a luminance term that the per-pixel variance of the mean
 * (k_moments.h) drives; the variance rides in the colour record's fourth lane.  The first filter's functions and kernels are not touched by it.
 */
#ifndef RPT_K_DENOISE_H
#define RPT_K_DENOISE_H

#include "k_shade.h"             /* load_material, sample_by_lod, the tri_shade records: the guides shade a hit as the shade stage does (k_shade itself is not instantiated) */
#include "k_tonemap.h"
#include "k_moments.h"           /* mo_luminance, mo_variance_of_mean: the variance-guided filter (dn_filter_pixel_var) */

#define RPT_DN_KIND_MISS 0u
#define RPT_DN_KIND_SURFACE 1u
#define RPT_DN_KIND_EMITTER 2u
#define RPT_DN_ALBEDO_FLOOR 0.01f
#define RPT_DN_MAX_ITERATIONS 6u
#define RPT_DN_MAX_NORMAL_POWER_LOG2 10u

/* what a pass needs of rpt_denoise_params, with the per-pass constants worked out once (the same f32 operations on the host and on the device) */
struct DnPass {
    uint32_t width, height;
    uint32_t step;                 /* 2^i */
    uint32_t normal_power_log2;
    float plane_scale;             /* (sigma_plane * step) * (2 / width): multiplied by the centre's depth it is the plane distance of one footprint */
    float sigma2;                  /* (sigma_color * 2^-i)^2; 0: the colour term is off */
};
RPT_HD DnPass dn_pass(uint32_t width, uint32_t height, uint32_t i, uint32_t normal_power_log2, float sigma_color, float sigma_plane) {
    DnPass p;
    p.width = width; p.height = height;
    p.step = 1u << i;
    p.normal_power_log2 = normal_power_log2;
    p.plane_scale = (sigma_plane * (float)p.step) * (2.0f / (float)width);
    const float sigma_i = sigma_color * rptm::u2f((127u - i) << 23);       /* 2^-i, exact */
    p.sigma2 = sigma_i * sigma_i;
    return p;
}

RPT_HD bool dn_finite3(F3 a) { return rptm::finiter(a.x) && rptm::finiter(a.y) && rptm::finiter(a.z); }
RPT_HD F3 dn_albedo_floor(F3 a) { return f3(rptm::fmaxr(a.x, RPT_DN_ALBEDO_FLOOR), rptm::fmaxr(a.y, RPT_DN_ALBEDO_FLOOR), rptm::fmaxr(a.z, RPT_DN_ALBEDO_FLOOR)); }
/* c / max(a, 0.01) per channel, and back */
RPT_HD F3 dn_demodulate(F3 c, F3 albedo) { const F3 a = dn_albedo_floor(albedo); return f3(c.x / a.x, c.y / a.y, c.z / a.z); }
RPT_HD F3 dn_remodulate(F3 e, F3 albedo) { return e * dn_albedo_floor(albedo); }

/* One pixel of one pass: sum(w e_q) / sum(w) over the 5 x 5 taps q = p + step * (dx, dy), dy outer, dx inner, both ascending, taps outside the image skipped.
 *   k     = h[dx] h[dy], h = {1/16, 1/4, 3/8, 1/4, 1/16} (the products are exact)
 *   w     = (k w_n) expr(-(d_x + d_c)); the centre tap counts with w = k = 9/64 whatever its guides say
 *   w = 0   if the kinds differ, if the tap's colour is not finite, or if w does not come out > 0 (a NaN from degenerate guides never enters a sum)
 *   w_n   = max(0, n_p . n_q), squared normal_power_log2 times            (both misses: 1)
 *   d_x   = |n_p . (x_q - x_p)| / (plane_scale t_p)                        (both misses: 0): the tap's distance from the centre's tangent plane in footprints
 *   d_c   = |e_p - e_q|^2 / (sigma2 ((|e_p|^2 + |e_q|^2) + 1e-12))         (sigma_color == 0: 0)
 * A centre that is not finite passes through unchanged, and so does one that no other tap joined ((k e) / k need not round back to e).  `colour`, `g0` = (normal | depth), `g1` = (position | kind) are row-major images. */
RPT_HD F3 dn_filter_pixel(const DnPass &ps, const float4 *colour, const float4 *g0, const float4 *g1, uint32_t x, uint32_t y) {
    const size_t at = (size_t)y * ps.width + x;
    const float4 cp = colour[at];
    const F3 e_p = f3(cp.x, cp.y, cp.z);
    if (!dn_finite3(e_p)) return e_p;
    const float4 a0 = g0[at], a1 = g1[at];
    const F3 n_p = f3(a0.x, a0.y, a0.z), x_p = f3(a1.x, a1.y, a1.z);
    const uint32_t kind_p = rptm::f2u(a1.w);
    const float plane = ps.plane_scale * a0.w;
    const float ep2 = dot3(e_p, e_p);
    F3 sum = f3s(0.0f);
    float wsum = 0.0f;
    bool joined = false;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = (int)y + dy * (int)ps.step;                                  /* (extents <= 65535, step <= 32) */
        if (qy < 0 || qy >= (int)ps.height) continue;
        const float hy = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = (int)x + dx * (int)ps.step;
            if (qx < 0 || qx >= (int)ps.width) continue;
            const float hx = dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f);
            const float k = hx * hy;
            F3 e_q = e_p;
            float w = k;
            if (dx != 0 || dy != 0) {
                const size_t aq = (size_t)qy * ps.width + (size_t)qx;
                const float4 b1 = g1[aq];
                if (rptm::f2u(b1.w) != kind_p) continue;
                const float4 cq = colour[aq];
                e_q = f3(cq.x, cq.y, cq.z);
                if (!dn_finite3(e_q)) continue;
                float w_n = 1.0f, d = 0.0f;
                if (kind_p != RPT_DN_KIND_MISS) {
                    const float4 b0 = g0[aq];
                    w_n = rptm::fmaxr(0.0f, dot3(n_p, f3(b0.x, b0.y, b0.z)));
                    for (uint32_t r = 0; r < ps.normal_power_log2; ++r) w_n = w_n * w_n;
                    d = rptm::absr(dot3(n_p, f3(b1.x, b1.y, b1.z) - x_p)) / plane;
                }
                if (ps.sigma2 != 0.0f) {
                    const F3 diff = e_p - e_q;
                    d = d + dot3(diff, diff) / (ps.sigma2 * ((ep2 + dot3(e_q, e_q)) + 1e-12f));
                }
                w = (k * w_n) * rptm::expr(-d);
                if (!(w > 0.0f)) continue;
                joined = true;
            }
            sum = sum + w * e_q;
            wsum = wsum + w;
        }
    }
    if (!joined) return e_p;
    return f3(sum.x / wsum, sum.y / wsum, sum.z / wsum);
}
/* after the last pass: back to radiance, then the display operator */
RPT_HD F3 dn_finish_pixel(F3 e, F3 albedo, bool demodulated, uint32_t tonemap_op) { return tonemap(tonemap_op, demodulated ? dn_remodulate(e, albedo) : e); }

/* ---- the variance-guided filter (rpt_denoise_variance): dn_filter_pixel with one more edge-stopping term, driven by the per-pixel variance of the mean
 * luminance that the moments record gives (k_moments.h mo_variance_of_mean; Schied et al. 2017).  The variance travels in the .w lane of the colour image
 * (a tap still reads 48 bytes) and is filtered along with the colour.  Its unit is that of the filtered luminance squared: radiance^2, or — with
 * demodulation — radiance^2 / Ya^2, Ya = the luminance of max(albedo, 0.01).  +inf stands for "unknown" (mo_variance_known). ------------------------------ */
struct DnVarOut { F3 e; float v; };

/* the pre-pass's variance of a pixel: the record's, divided by Ya^2 where the mean was demodulated (an unknown one stays unknown) */
RPT_HD float dn_prepare_variance(const float4 &m, bool demodulated, F3 albedo) {
    float v = mo_variance_of_mean(m);
    if (demodulated && mo_variance_known(v)) {
        const F3 a = dn_albedo_floor(albedo);
        const float Ya = mo_luminance(a.x, a.y, a.z);
        v = v / (Ya * Ya);
    }
    return v;
}

/* vbar_p: the 3 x 3 Gaussian {1/4, 1/2, 1/4}^2 of the pass's INPUT variance around p, taps at distance 1 whatever the pass's step, dy outer, dx inner, both
 * ascending, over the taps that are inside the image, of p's kind and of known variance (the centre is one of them when its variance is known), divided by
 * the sum of the kernel weights used (the products and their sums are exact).  No tap: unknown. */
RPT_HD float dn_prefilter_variance(const DnPass &ps, const float4 *colour, const float4 *g1, uint32_t x, uint32_t y, uint32_t kind_p) {
    float acc = 0.0f, ksum = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = (int)y + dy;
        if (qy < 0 || qy >= (int)ps.height) continue;
        const float hy = dy == 0 ? 0.5f : 0.25f;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = (int)x + dx;
            if (qx < 0 || qx >= (int)ps.width) continue;
            const size_t aq = (size_t)qy * ps.width + (size_t)qx;
            if (rptm::f2u(g1[aq].w) != kind_p) continue;
            const float v_q = colour[aq].w;
            if (!mo_variance_known(v_q)) continue;
            const float k = (dx == 0 ? 0.5f : 0.25f) * hy;
            acc = acc + k * v_q;
            ksum = ksum + k;
        }
    }
    return ksum > 0.0f ? acc / ksum : rptm::u2f(0x7f800000u);
}

/* One pixel of one pass of the variance-guided filter: dn_filter_pixel, every rule of it, and
 *   d_l   = |Y(e_p) - Y(e_q)| / (sigma_variance sqrt(vbar_p) + 1e-6)        Y = mo_luminance; added to d after d_c: w = (k w_n) expr(-(d_x + d_c + d_l))
 * when sigma_variance != 0 and vbar_p is known; otherwise NO term is added and the colour is dn_filter_pixel's, bit for bit.
 * The variance that goes out with the colour is sum(w^2 v_q) / sum(w)^2 over the taps that joined and whose variance is known, the centre (w = 9/64)
 * included; it is known iff the centre's was.  A pixel that passes through unchanged keeps its variance. */
RPT_HD DnVarOut dn_filter_pixel_var(const DnPass &ps, float sigma_variance, const float4 *colour, const float4 *g0, const float4 *g1, uint32_t x, uint32_t y) {
    const size_t at = (size_t)y * ps.width + x;
    const float4 cp = colour[at];
    const F3 e_p = f3(cp.x, cp.y, cp.z);
    const float v_p = cp.w;
    if (!dn_finite3(e_p)) return DnVarOut{e_p, v_p};
    const float4 a0 = g0[at], a1 = g1[at];
    const F3 n_p = f3(a0.x, a0.y, a0.z), x_p = f3(a1.x, a1.y, a1.z);
    const uint32_t kind_p = rptm::f2u(a1.w);
    const float plane = ps.plane_scale * a0.w;
    const float ep2 = dot3(e_p, e_p);
    bool lum_term = false;
    float lum_width = 0.0f, Y_p = 0.0f;
    if (sigma_variance != 0.0f) {
        const float vbar = dn_prefilter_variance(ps, colour, g1, x, y, kind_p);
        if (mo_variance_known(vbar)) {
            lum_term = true;
            lum_width = sigma_variance * rptm::sqrtr(vbar) + 1e-6f;
            Y_p = mo_luminance(e_p.x, e_p.y, e_p.z);
        }
    }
    F3 sum = f3s(0.0f);
    float wsum = 0.0f, vsum = 0.0f;
    bool joined = false;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = (int)y + dy * (int)ps.step;
        if (qy < 0 || qy >= (int)ps.height) continue;
        const float hy = dy == 0 ? 0.375f : ((dy == 1 || dy == -1) ? 0.25f : 0.0625f);
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = (int)x + dx * (int)ps.step;
            if (qx < 0 || qx >= (int)ps.width) continue;
            const float hx = dx == 0 ? 0.375f : ((dx == 1 || dx == -1) ? 0.25f : 0.0625f);
            const float k = hx * hy;
            F3 e_q = e_p;
            float w = k, v_q = v_p;
            if (dx != 0 || dy != 0) {
                const size_t aq = (size_t)qy * ps.width + (size_t)qx;
                const float4 b1 = g1[aq];
                if (rptm::f2u(b1.w) != kind_p) continue;
                const float4 cq = colour[aq];
                e_q = f3(cq.x, cq.y, cq.z);
                v_q = cq.w;
                if (!dn_finite3(e_q)) continue;
                float w_n = 1.0f, d = 0.0f;
                if (kind_p != RPT_DN_KIND_MISS) {
                    const float4 b0 = g0[aq];
                    w_n = rptm::fmaxr(0.0f, dot3(n_p, f3(b0.x, b0.y, b0.z)));
                    for (uint32_t r = 0; r < ps.normal_power_log2; ++r) w_n = w_n * w_n;
                    d = rptm::absr(dot3(n_p, f3(b1.x, b1.y, b1.z) - x_p)) / plane;
                }
                if (ps.sigma2 != 0.0f) {
                    const F3 diff = e_p - e_q;
                    d = d + dot3(diff, diff) / (ps.sigma2 * ((ep2 + dot3(e_q, e_q)) + 1e-12f));
                }
                if (lum_term) d = d + rptm::absr(Y_p - mo_luminance(e_q.x, e_q.y, e_q.z)) / lum_width;
                w = (k * w_n) * rptm::expr(-d);
                if (!(w > 0.0f)) continue;
                joined = true;
            }
            sum = sum + w * e_q;
            wsum = wsum + w;
            if (mo_variance_known(v_q)) vsum = vsum + (w * w) * v_q;
        }
    }
    if (!joined) return DnVarOut{e_p, v_p};
    return DnVarOut{f3(sum.x / wsum, sum.y / wsum, sum.z / wsum), mo_variance_known(v_p) ? vsum / (wsum * wsum) : rptm::u2f(0x7f800000u)};
}

/* ---- guides ------------------------------------------------------------------------------------------------------------------------------------------ */
/* camera_ray (k_path.h, lib.rs:36-51) through the pixel CENTRE: the jitter replaced by (0.5, 0.5) */
__device__ __forceinline__ void camera_ray_centre(const DevConfig &cfg, uint32_t px, uint32_t py, F3 &ro, F3 &rd) {
    float sx = (float)px + 0.5f, sy = (float)py + 0.5f;
    float ux = (sx / (float)cfg.c.width) * 2.0f - 1.0f;
    float uy = (1.0f - sy / (float)cfg.c.height) * 2.0f - 1.0f;
    uy *= (float)cfg.c.height / (float)cfg.c.width;
    ro = f3(cfg.c.cam_position[0], cfg.c.cam_position[1], cfg.c.cam_position[2]);
    rd = mat3_mul(cfg.euler, norm3(f3(ux, uy, 1.0f)));
}

/* ray i = the centre ray of pixel order[i] (x | y << 16): the tile order of the whole image, so a wave walks an 8 x 8 pixel block as it does for primary rays */
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_camera_rays(DevConfig cfg, const uint32_t *order, uint32_t n, float *origins, float *dirs) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t pxy = order[i];
    F3 ro, rd;
    camera_ray_centre(cfg, pxy & 0xffffu, pxy >> 16, ro, rd);
    const size_t j = 3u * (size_t)i;
    origins[j] = ro.x; origins[j + 1u] = ro.y; origins[j + 2u] = ro.z;
    dirs[j] = rd.x; dirs[j + 1u] = rd.y; dirs[j + 2u] = rd.z;
}

/* the hit of ray i (t, triangle, flags bit 0 = hit: the outputs of the one-ray-per-lane nearest-hit walk) shaded into the guide records of its pixel */
template <bool TEXTURED>
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_shade_guides(DevScene sc, uint32_t width, const uint32_t *order, uint32_t n, const float *origins, const float *dirs,
                                                               const float *hit_t, const uint32_t *hit_tri, const uint32_t *hit_flags, float4 *g0, float4 *g1, float4 *albedo_out) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t pxy = order[i];
    const size_t at = rpt_pixel_index(pxy, width);
    const size_t j = 3u * (size_t)i;
    const F3 ro = f3(origins[j], origins[j + 1u], origins[j + 2u]), rd = f3(dirs[j], dirs[j + 1u], dirs[j + 2u]);
    const float t = hit_t[i];
    const F3 hit = ro + rd * t;                                                     /* lib.rs:64 (a miss leaves t = 1e6) */
    uint32_t kind = RPT_DN_KIND_MISS;
    F3 albedo = f3s(1.0f), normal = f3s(0.0f);
    if ((hit_flags[i] & 1u) != 0u) {
        const uint32_t tri_index = hit_tri[i];
        const float4 *ts = sc.tri_shade + 4u * tri_index;
        const float4 s0 = ts[0], s1 = ts[1], s2 = ts[2];
        const Mat mat = load_material<TEXTURED>(sc, __float_as_uint(s2.w));
        const bool emits = mat.emissive.x != 0.0f || mat.emissive.y != 0.0f || mat.emissive.z != 0.0f;
        kind = emits ? RPT_DN_KIND_EMITTER : RPT_DN_KIND_SURFACE;
        /* interpolation as the shade stage does it (k_shade.h shade_slot, lib.rs:112-141) */
        const float4 *tg = sc.tri_geom + 3u * tri_index;
        const float4 q0 = tg[0], q1 = tg[1], q2 = tg[2];
        F3 bary;
        {
            F3 v0 = xyz4(q1), v1 = xyz4(q2), v2 = hit - xyz4(q0);
            float d00 = q0.w, d01 = q1.w, d11 = q2.w;
            float d20 = dot3(v2, v0), d21 = dot3(v2, v1);
            float denom = d00 * d11 - d01 * d01;
            float v = (d11 * d20 - d01 * d21) / denom;
            float w = (d00 * d21 - d01 * d20) / denom;
            bary = f3(1.0f - v - w, v, w);
        }
        normal = bary.x * xyz4(s0) + bary.y * xyz4(s1) + bary.z * xyz4(s2);
        if (!emits) albedo = xyz4(mat.albedo);
        if (TEXTURED) {
            const float4 s3 = ts[3];
            float uv_x = (bary.x * s0.w + bary.y * s3.x) + bary.z * s3.z;
            float uv_y = (bary.x * s1.w + bary.y * s3.y) + bary.z * s3.w;
            float cx = rptm::fminr(rptm::fmaxr(uv_x, 0.0f), 1.0f), cy = rptm::fminr(rptm::fmaxr(uv_y, 0.0f), 1.0f);
            if (cx != uv_x || cy != uv_y) {
                uv_x = uv_x - rptm::floorr(uv_x);
                uv_y = uv_y - rptm::floorr(uv_y);
            }
            if (mat.has.w != 0u) {
                float4 s = sample_by_lod<true>(sc.atlas, mat.normals.x + uv_x * mat.normals.z, mat.normals.y + uv_y * mat.normals.w);
                F3 nm = f3(s.x * 2.0f - 1.0f, s.y * 2.0f - 1.0f, s.z * 2.0f - 1.0f);
                const float4 *tt = sc.tri_tangent + 3u * tri_index;
                F3 tangent = bary.x * xyz4(tt[0]) + bary.y * xyz4(tt[1]) + bary.z * xyz4(tt[2]);
                F3 bitangent = cross3(tangent, normal);
                F3 r = tangent * nm.x;
                r = r + (bitangent * nm.y);
                r = r + (normal * nm.z);
                normal = norm3(r);                                                  /* lib.rs:141 normalises the mapped normal; the guide normalises again below */
            }
            if (!emits && mat.has.x != 0u) {
                float4 s = sample_by_lod<true>(sc.atlas, mat.albedo.x + uv_x * mat.albedo.z, mat.albedo.y + uv_y * mat.albedo.w);
                albedo = f3(s.x, s.y, s.z);
            }
        }
        normal = norm3(normal);
        if (!finite3(normal)) normal = f3s(0.0f);                                   /* a zero vector normalises to NaN */
    }
    g0[at] = make_float4(normal.x, normal.y, normal.z, t);
    g1[at] = make_float4(hit.x, hit.y, hit.z, __uint_as_float(kind));
    albedo_out[at] = make_float4(albedo.x, albedo.y, albedo.z, 0.0f);
}

/* ---- filter ------------------------------------------------------------------------------------------------------------------------------------------ */
/* pre-pass: mean = sum.rgb / samples (bit for bit the mean of rpt_resolve op 0), demodulated where asked, into row-major order.  `order` != null: element i
 * of `sums` is pixel order[i] (the context's tile-major accumulator); null: `sums` is row-major already (a gathered image). */
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_prepare(const float4 *sums, const uint32_t *order, uint32_t n, uint32_t width, float sample_count, const float4 *albedo /* null: no demodulation */,
                                                          float4 *out) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    size_t at = i;
    if (order) at = rpt_pixel_index(order[i], width);
    const float4 a = sums[i];
    F3 c = f3(a.x / sample_count, a.y / sample_count, a.z / sample_count);
    if (albedo) c = dn_demodulate(c, xyz4(albedo[at]));
    out[at] = make_float4(c.x, c.y, c.z, 0.0f);
}

/* one pass, one thread per pixel; LAST: the finish (remodulation, display operator, RGB out) is fused in.  A wave is a 64 x 1 row segment, a workgroup 64 x 4
 * pixels: every load of a tap row is one contiguous KiB at any step.  (A wave as an 8 x 8 block was measured too and is slower at every step:
 * profiles/r11_denoise.txt.) */
template <bool LAST>
__global__ __launch_bounds__(256) void k_dn_pass(DnPass ps, const float4 *src, const float4 *g0, const float4 *g1, float4 *dst, const float4 *albedo, uint32_t demodulated,
                                                 uint32_t tonemap_op, float *out_rgb) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= ps.width || y >= ps.height) return;
    const F3 e = dn_filter_pixel(ps, src, g0, g1, x, y);
    const size_t at = (size_t)y * ps.width + x;
    if (LAST) {
        const F3 c = dn_finish_pixel(e, xyz4(albedo[at]), demodulated != 0u, tonemap_op);
        out_rgb[3u * at] = c.x; out_rgb[3u * at + 1u] = c.y; out_rgb[3u * at + 2u] = c.z;
    } else {
        dst[at] = make_float4(e.x, e.y, e.z, 0.0f);
    }
}

/* iterations == 0: the prepared mean through the display operator — what rpt_resolve writes */
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_resolve(const float4 *mean, uint32_t n, uint32_t tonemap_op, float *out_rgb) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const F3 c = tonemap(tonemap_op, xyz4(mean[i]));
    const size_t j = 3u * (size_t)i;
    out_rgb[j] = c.x; out_rgb[j + 1u] = c.y; out_rgb[j + 2u] = c.z;
}

/* ---- the variance-guided filter's kernels (rpt_denoise_variance) ------------------------------------------------------------------------------------- */
/* one pass, the mapping of k_dn_pass (a wave a 64 x 1 row segment, a workgroup 64 x 4 pixels).  The nine step-1 variance reads of neighbouring lanes
 * overlap and are left to the cache: at step 1 they are taps of the 5 x 5 loop, at every step they are rows the workgroup reads as whole lines. */
template <bool LAST>
__global__ __launch_bounds__(256) void k_dn_pass_var(DnPass ps, float sigma_variance, const float4 *src, const float4 *g0, const float4 *g1, float4 *dst, const float4 *albedo,
                                                     uint32_t demodulated, uint32_t tonemap_op, float *out_rgb, float *out_variance) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    if (x >= ps.width || y >= ps.height) return;
    const DnVarOut o = dn_filter_pixel_var(ps, sigma_variance, src, g0, g1, x, y);
    const size_t at = (size_t)y * ps.width + x;
    if (LAST) {
        const F3 c = dn_finish_pixel(o.e, xyz4(albedo[at]), demodulated != 0u, tonemap_op);
        out_rgb[3u * at] = c.x; out_rgb[3u * at + 1u] = c.y; out_rgb[3u * at + 2u] = c.z;
        out_variance[at] = o.v;
    } else {
        dst[at] = make_float4(o.e.x, o.e.y, o.e.z, o.v);
    }
}

/* iterations == 0: the prepared variance as a plane (the colour goes through k_dn_resolve) */
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_variance_plane(const float4 *mean, uint32_t n, float *out_variance) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    out_variance[i] = mean[i].w;
}

/* rpt_read_guides: the packed records as the planes a caller (OIDN's auxiliary images, the tests) takes; every destination nullable */
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_unpack_guides(const float4 *g0, const float4 *g1, const float4 *albedo, uint32_t n, float *albedo_rgb, float *normal_xyz, float *depth,
                                                                float *position_xyz, uint32_t *kind) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 a0 = g0[i], a1 = g1[i], al = albedo[i];
    const size_t j = 3u * (size_t)i;
    if (albedo_rgb) { albedo_rgb[j] = al.x; albedo_rgb[j + 1u] = al.y; albedo_rgb[j + 2u] = al.z; }
    if (normal_xyz) { normal_xyz[j] = a0.x; normal_xyz[j + 1u] = a0.y; normal_xyz[j + 2u] = a0.z; }
    if (depth) depth[i] = a0.w;
    if (position_xyz) { position_xyz[j] = a1.x; position_xyz[j + 1u] = a1.y; position_xyz[j + 2u] = a1.z; }
    if (kind) kind[i] = __float_as_uint(a1.w);
}

#endif /* RPT_K_DENOISE_H */
