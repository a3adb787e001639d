/*
 * k_guides_glass.h — denoiser guides that follow glass to the surface seen through it (include/rpt/rpt.h rpt_set_guides_through_glass).  Opt-in, beside the
 * first-hit guides of k_denoise.h: with the setting at 0, or while no material record is Glass, nothing of this header is launched.
 *
 * With K = max_interfaces > 0 the guide of a pixel is the end of a deterministic chain that starts at the pixel's centre ray and continues through every hit
 * on a material whose record is RPT_MODEL_GLASS, along the lobe Glass::sample (bsdf.rs:128-165) takes more often at zero roughness — the reflection where the
 * Schlick term is above 1/2, else the refraction — with the guide's normalised shading normal as the microsurface normal (the tracer hands its BSDF the
 * un-normalised one, lib.rs:125: the chain is a guide, not a sample).  One round = one walk of the rays still inside glass + one step per ray; at most K + 1
 * rounds.  The chain carries the product A of the albedos of the interfaces it was refracted through, the summed hit distances L (the origin moves by
 * dir * EPS per interface, lib.rs:172; L sums the t only) and the number of interfaces m.  The records of the final hit:
 *     g0 = (normal | L)     g1 = (ro0 + rd0 * L | kind)     albedo = (A * a | 0)
 * — the position is the point at optical path length L UNFOLDED ALONG THE PRIMARY RAY, so that it lies on the pixel's own ray (k_temporal.h inverts the
 * pinhole camera in closed form) and plane_scale * L stays the pixel's footprint.  Kinds stay {0, 1, 2}.  A chain that meets no glass is the first-hit guide,
 * byte for byte: L = 0 + t, A * a = 1 * a.
 *
 * The per-ray arithmetic is ONE RPT_HD function, dn_glass_step — f32, no contraction, rptm:: math, IEEE division — that the device kernel and the host hook
 * (rpt_debug_glass_step_host) both call; tests/guides_glass_ref.py restates it in numpy with the same operation order.  The hit shading of k_dn_shade_guides
 * is restated here as RPT_HD text (that kernel's helpers are device functions, and it keeps its instruction stream).
 *
 * Between rounds the rays still inside glass are compacted in ASCENDING ray index — count per workgroup (inside the step kernel), exclusive scan, scatter: the
 * scheme of k_adaptive.h — so an 8 x 8 pixel block's rays stay together in a wave and nothing depends on the order waves arrive in.
 */
#ifndef RPT_K_GUIDES_GLASS_H
#define RPT_K_GUIDES_GLASS_H

#include "k_denoise.h"

#define RPT_GG_MAX_INTERFACES 8u

/* what a step reads of the scene: the records of DevScene by the same names (the host hook builds them for the triangle at hand), the atlas as RGBA8 words */
struct GgScene {
    const float4 *tri_geom, *tri_shade, *tri_tangent, *materials, *mat_lite;
    const uint32_t *atlas;
    uint32_t atlas_w, atlas_h;
};

/* the chain of a pixel between two rounds */
struct GgChain {
    F3 A;                  /* product of the albedos of the interfaces refracted through; starts at (1, 1, 1) */
    float L;               /* summed hit distances; starts at 0 */
    uint32_t m;            /* interfaces crossed; starts at 0 */
};

struct GgStep {
    bool final;            /* the records below are the pixel's; else (ro, rd, chain) go into the next round */
    bool exhausted;        /* final on a glass surface: the budget, a zero normal or a direction that is not finite */
    uint32_t kind;
    F3 normal, albedo;
    F3 ro, rd;
    GgChain chain;         /* final: .L is the guide's depth, .m the interfaces the chain crossed */
};

RPT_HD F3 gg_xyz(const float4 &v) { return f3(v.x, v.y, v.z); }
RPT_HD F3 gg_cross(F3 a, F3 b) { return f3(a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y); }
RPT_HD F3 gg_norm(F3 a) { return a * rptm::rcp_rn(rptm::sqrtr(dot3(a, a))); }

/* sample_by_lod<true> (k_shade.h; image_polyfill.rs:32-55) on the RGBA8 atlas, texel by texel */
RPT_HD uint32_t gg_wrap(int32_t c, uint32_t extent) {                              /* image_wrap: the sign-extended coordinate's unsigned 64-bit remainder */
    const uint32_t u = (uint32_t)c;
    if (u < extent) return u;
    if (u == extent) return 0u;
    return (uint32_t)((uint64_t)(int64_t)c % (uint64_t)extent);
}
RPT_HD F3 gg_texel(uint32_t t) { return f3(rptm::unorm8((float)(t & 0xffu)), rptm::unorm8((float)((t >> 8) & 0xffu)), rptm::unorm8((float)((t >> 16) & 0xffu))); }
RPT_HD F3 gg_lerp(F3 a, F3 b, float s) { return f3(a.x + ((b.x - a.x) * s), a.y + ((b.y - a.y) * s), a.z + ((b.z - a.z) * s)); }
RPT_HD F3 gg_sample_atlas(const GgScene &sc, float u, float v) {
    const float sx = u * (float)sc.atlas_w, sy = v * (float)sc.atlas_h;
    const float fx = rptm::floorr(sx), fy = rptm::floorr(sy);
    const float tx = sx - fx, ty = sy - fy;
    const uint32_t x0 = gg_wrap(rptm::f2i32_sat(fx), sc.atlas_w), x1 = gg_wrap(rptm::f2i32_sat(rptm::ceilr(sx)), sc.atlas_w);
    const uint32_t y0 = gg_wrap(rptm::f2i32_sat(fy), sc.atlas_h), y1 = gg_wrap(rptm::f2i32_sat(rptm::ceilr(sy)), sc.atlas_h);
    const F3 c00 = gg_texel(sc.atlas[y0 * sc.atlas_w + x0]), c10 = gg_texel(sc.atlas[y0 * sc.atlas_w + x1]);      /* (an image has at most 2^30 texels: rpt_upload_scene) */
    const F3 c01 = gg_texel(sc.atlas[y1 * sc.atlas_w + x0]), c11 = gg_texel(sc.atlas[y1 * sc.atlas_w + x1]);
    return gg_lerp(gg_lerp(c00, c10, tx), gg_lerp(c01, c11, tx), ty);
}

/* One step of the chain on plain values: the current ray, its nearest hit (t, triangle, hit or miss), the chain so far.  `models`: one (model, ior bits, -, -)
 * per material, or null for "every material is PBR".  K: the budget of interfaces. */
template <bool TEXTURED>
RPT_HD GgStep dn_glass_step(const GgScene &sc, const uint4 *models, uint32_t K, F3 ro, F3 rd, float t, uint32_t tri_index, bool is_hit, GgChain ch) {
    GgStep o;
    o.final = true; o.exhausted = false;
    o.kind = RPT_DN_KIND_MISS;
    o.normal = f3s(0.0f); o.albedo = ch.A;
    o.ro = ro; o.rd = rd;
    o.chain = ch;
    if (!is_hit) {
        o.chain.L = ch.L + 1e6f;
        return o;
    }
    const F3 hit = ro + rd * t;                                                     /* lib.rs:64 */
    o.chain.L = ch.L + t;                                                           /* (the origin's dir * EPS shifts are not part of L) */
    /* the hit shaded as k_dn_shade_guides shades it */
    const float4 *ts = sc.tri_shade + 4u * (size_t)tri_index;
    const float4 s0 = ts[0], s1 = ts[1], s2 = ts[2];
    const uint32_t mat_index = rptm::f2u(s2.w);
    F3 emissive, mat_albedo;
    float4 mat_albedo4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), mat_normals4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool has_albedo = false, has_normal = false;
    if (TEXTURED) {
        const float4 *p = sc.materials + 6u * (size_t)mat_index;
        emissive = gg_xyz(p[0]);
        mat_albedo4 = p[1]; mat_normals4 = p[4];
        mat_albedo = gg_xyz(mat_albedo4);
        has_albedo = rptm::f2u(p[5].x) != 0u; has_normal = rptm::f2u(p[5].w) != 0u;
    } else {
        const float4 *p = sc.mat_lite + 2u * (size_t)mat_index;
        emissive = gg_xyz(p[0]);
        mat_albedo = gg_xyz(p[1]);
    }
    const bool emits = emissive.x != 0.0f || emissive.y != 0.0f || emissive.z != 0.0f;
    const float4 *tg = sc.tri_geom + 3u * (size_t)tri_index;
    const float4 q0 = tg[0], q1 = tg[1], q2 = tg[2];
    F3 bary;
    {
        const F3 v0 = gg_xyz(q1), v1 = gg_xyz(q2), v2 = hit - gg_xyz(q0);
        const float d00 = q0.w, d01 = q1.w, d11 = q2.w;
        const float d20 = dot3(v2, v0), d21 = dot3(v2, v1);
        const float denom = d00 * d11 - d01 * d01;
        const float v = (d11 * d20 - d01 * d21) / denom;
        const float w = (d00 * d21 - d01 * d20) / denom;
        bary = f3(1.0f - v - w, v, w);
    }
    F3 normal = bary.x * gg_xyz(s0) + bary.y * gg_xyz(s1) + bary.z * gg_xyz(s2);
    F3 a = emits ? f3s(1.0f) : mat_albedo;
    if (TEXTURED) {
        const float4 s3 = ts[3];
        float uv_x = (bary.x * s0.w + bary.y * s3.x) + bary.z * s3.z;
        float uv_y = (bary.x * s1.w + bary.y * s3.y) + bary.z * s3.w;
        const float cx = rptm::fminr(rptm::fmaxr(uv_x, 0.0f), 1.0f), cy = rptm::fminr(rptm::fmaxr(uv_y, 0.0f), 1.0f);
        if (cx != uv_x || cy != uv_y) {
            uv_x = uv_x - rptm::floorr(uv_x);
            uv_y = uv_y - rptm::floorr(uv_y);
        }
        if (has_normal) {
            const F3 s = gg_sample_atlas(sc, mat_normals4.x + uv_x * mat_normals4.z, mat_normals4.y + uv_y * mat_normals4.w);
            const F3 nm = f3(s.x * 2.0f - 1.0f, s.y * 2.0f - 1.0f, s.z * 2.0f - 1.0f);
            const float4 *tt = sc.tri_tangent + 3u * (size_t)tri_index;
            const F3 tangent = bary.x * gg_xyz(tt[0]) + bary.y * gg_xyz(tt[1]) + bary.z * gg_xyz(tt[2]);
            const F3 bitangent = gg_cross(tangent, normal);
            F3 r = tangent * nm.x;
            r = r + (bitangent * nm.y);
            r = r + (normal * nm.z);
            normal = gg_norm(r);
        }
        if (!emits && has_albedo) a = gg_sample_atlas(sc, mat_albedo4.x + uv_x * mat_albedo4.z, mat_albedo4.y + uv_y * mat_albedo4.w);
    }
    normal = gg_norm(normal);
    if (!dn_finite3(normal)) normal = f3s(0.0f);                                    /* a zero vector normalises to NaN */
    const F3 Aa = ch.A * a;
    o.kind = emits ? RPT_DN_KIND_EMITTER : RPT_DN_KIND_SURFACE;
    o.normal = normal; o.albedo = Aa;
    uint4 model = make_uint4(0u, 0u, 0u, 0u);
    if (models) model = models[mat_index];
    if (emits || model.x != RPT_DEV_MODEL_GLASS) return o;                          /* an emitter, another model, no records: the chain ends here */
    o.kind = RPT_DN_KIND_SURFACE;
    o.exhausted = true;
    if (ch.m >= K || (normal.x == 0.0f && normal.y == 0.0f && normal.z == 0.0f)) return o;
    /* Glass::sample at zero roughness with the microsurface normal = the shading normal (k_bsdf_extra.h glass_sample, the same operations in the same order) */
    const float ior = rptm::u2f(model.y);
    const F3 view = -rd;
    const bool inside = dot3(normal, view) < 0.0f;
    const F3 nrm = inside ? -normal : normal;
    const float in_ior = inside ? ior : 1.0f, out_ior = inside ? 1.0f : ior;
    const float c = dot3(view, nrm);
    float f0 = (in_ior - out_ior) / (in_ior + out_ior);
    f0 = f0 * f0;
    const float fresnel = f0 + (1.0f - f0) * rptm::powi5(1.0f - rptm::fmaxr(c, 0.0f));
    F3 dir, A = ch.A;
    if (fresnel > 0.5f) {
        dir = gg_norm(2.0f * rptm::absr(c) * nrm - view);
    } else {
        const float eta = in_ior / out_ior;
        const float sg = c != c ? c : ((rptm::f2u(c) >> 31) ? -1.0f : 1.0f);       /* f32::signum: +1 for +0, -1 for -0 */
        dir = gg_norm((eta * c - sg * rptm::sqrtr(rptm::fmaxr(1.0f + eta * (c * c - 1.0f), 0.0f))) * nrm - eta * view);
        A = Aa;
    }
    if (!dn_finite3(dir)) return o;                                                 /* as if the budget were exhausted */
    o.final = false; o.exhausted = false;
    o.ro = hit + dir * RPT_EPS;                                                     /* lib.rs:172 */
    o.rd = dir;
    o.chain.A = A;
    o.chain.m = ch.m + 1u;
    return o;
}

/* ---- device ------------------------------------------------------------------------------------------------------------------------------------------ */
/* what a build reports to the host: n_active is the one read per round (the scan writes it); the two counts grow as chains end (one integer atomic per wave) */
struct GgResult {
    uint32_t n_active;
    uint32_t crossed;              /* pixels whose chain crossed at least one interface */
    uint32_t exhausted;            /* pixels whose chain ended on a glass surface */
    uint32_t pad;
};

/* the arrays of one round: ray i of the round belongs to pixel slot[i] of the tile order (null: i itself, the first round) */
struct GgRays {
    const float *origins, *dirs;
    const uint32_t *slot;
    const float *hit_t;
    const uint32_t *hit_tri, *hit_flags;
};
/* where a ray that goes on is written (at its own index; the scatter compacts), and the chains, by pixel slot */
struct GgNext {
    float *origins, *dirs;
    uint32_t *slot;
    float4 *chain;                 /* (A | L) */
    uint32_t *interfaces;          /* m */
    uint8_t *flags;                /* 1: the ray goes on */
    uint32_t *wg_count;            /* the workgroup's number of such rays */
};

/* One lane per active ray: the final records of its pixel, or its next ray and chain.  first: the chains are the initial ones and are not read.  Every lane
 * reaches the ballot: no early return.  LDS: 16 bytes. */
template <bool TEXTURED>
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_glass_step(GgScene sc, const uint4 *models, uint32_t K, uint32_t first, uint32_t width, const uint32_t *order, uint32_t n,
                                                             GgRays in, const float *origins0, const float *dirs0, GgNext next, float4 *g0, float4 *g1, float4 *albedo_out,
                                                             GgResult *res) {
    __shared__ uint32_t wave_n[RPT_BLOCK / RPT_WAVE];
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    bool goes_on = false, crossed = false, exhausted = false;
    if (i < n) {
        const uint32_t s = in.slot ? in.slot[i] : i;
        const size_t j = 3u * (size_t)i;
        GgChain ch{f3s(1.0f), 0.0f, 0u};
        if (first == 0u) {
            const float4 c4 = next.chain[s];
            ch = GgChain{f3(c4.x, c4.y, c4.z), c4.w, next.interfaces[s]};
        }
        const GgStep o = dn_glass_step<TEXTURED>(sc, models, K, f3(in.origins[j], in.origins[j + 1u], in.origins[j + 2u]), f3(in.dirs[j], in.dirs[j + 1u], in.dirs[j + 2u]),
                                                 in.hit_t[i], in.hit_tri[i], (in.hit_flags[i] & 1u) != 0u, ch);
        if (o.final) {
            const size_t at = rpt_pixel_index(order[s], width), j0 = 3u * (size_t)s;
            const F3 x = f3(origins0[j0], origins0[j0 + 1u], origins0[j0 + 2u]) + f3(dirs0[j0], dirs0[j0 + 1u], dirs0[j0 + 2u]) * o.chain.L;
            g0[at] = make_float4(o.normal.x, o.normal.y, o.normal.z, o.chain.L);
            g1[at] = make_float4(x.x, x.y, x.z, rptm::u2f(o.kind));
            albedo_out[at] = make_float4(o.albedo.x, o.albedo.y, o.albedo.z, 0.0f);
            crossed = o.chain.m != 0u;
            exhausted = o.exhausted;
        } else {
            goes_on = true;
            next.origins[j] = o.ro.x; next.origins[j + 1u] = o.ro.y; next.origins[j + 2u] = o.ro.z;
            next.dirs[j] = o.rd.x; next.dirs[j + 1u] = o.rd.y; next.dirs[j + 2u] = o.rd.z;
            next.slot[i] = s;
            next.chain[s] = make_float4(o.chain.A.x, o.chain.A.y, o.chain.A.z, o.chain.L);
            next.interfaces[s] = o.chain.m;
        }
        next.flags[i] = goes_on ? 1u : 0u;
    }
    const unsigned long long m = rpt_ballot(goes_on), mc = rpt_ballot(crossed), me = rpt_ballot(exhausted);
    if ((threadIdx.x & (RPT_WAVE - 1u)) == 0u) {
        wave_n[threadIdx.x / RPT_WAVE] = (uint32_t)__popcll(m);
        if (mc != 0ull) atomicAdd(&res->crossed, (uint32_t)__popcll(mc));
        if (me != 0ull) atomicAdd(&res->exhausted, (uint32_t)__popcll(me));
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (uint32_t w = 0; w < RPT_BLOCK / RPT_WAVE; ++w) total += wave_n[w];
        next.wg_count[blockIdx.x] = total;
    }
}

/* exclusive scan of the workgroup counts by ONE workgroup, and their total: n_active (k_adaptive.h k_ad_scan, on this header's result record) */
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_glass_scan(const uint32_t *wg_count, uint32_t n_blocks, uint32_t *wg_offset, GgResult *res) {
    __shared__ uint32_t part[RPT_BLOCK];
    const uint32_t per = (n_blocks + RPT_BLOCK - 1u) / RPT_BLOCK;
    const uint32_t lo = threadIdx.x * per < n_blocks ? threadIdx.x * per : n_blocks, hi = lo + per < n_blocks ? lo + per : n_blocks;
    uint32_t sum = 0u;
    for (uint32_t i = lo; i < hi; ++i) sum += wg_count[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t running = 0u;
        for (uint32_t t = 0; t < RPT_BLOCK; ++t) {
            const uint32_t v = part[t];
            part[t] = running;
            running += v;
        }
        res->n_active = running;
    }
    __syncthreads();
    uint32_t at = part[threadIdx.x];
    for (uint32_t i = lo; i < hi; ++i) {
        wg_offset[i] = at;
        at += wg_count[i];
    }
}

/* flagged ray i becomes ray r of the next round, r = the flagged rays below i.  capacity: what the destination holds (>= n_active, checked all the same) */
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_glass_scatter(uint32_t n, const uint8_t *flags, const uint32_t *wg_offset, uint32_t capacity, const float *origins, const float *dirs,
                                                                const uint32_t *slot, float *origins_out, float *dirs_out, uint32_t *slot_out) {
    __shared__ uint32_t wave_n[RPT_BLOCK / RPT_WAVE];
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x, wave = threadIdx.x / RPT_WAVE;
    const bool flag = i < n && flags[i] != 0u;
    const unsigned long long m = rpt_ballot(flag);
    if ((threadIdx.x & (RPT_WAVE - 1u)) == 0u) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t r = wg_offset[blockIdx.x] + rpt_lane_rank(m);
    for (uint32_t w = 0; w < wave; ++w) r += wave_n[w];
    if (!flag || r >= capacity) return;
    const size_t j = 3u * (size_t)i, k = 3u * (size_t)r;
    origins_out[k] = origins[j]; origins_out[k + 1u] = origins[j + 1u]; origins_out[k + 2u] = origins[j + 2u];
    dirs_out[k] = dirs[j]; dirs_out[k + 1u] = dirs[j + 1u]; dirs_out[k + 2u] = dirs[j + 2u];
    slot_out[r] = slot[i];
}

#endif /* RPT_K_GUIDES_GLASS_H */
