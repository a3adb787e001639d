/*
 * rpt_denoise.hip — the denoise step behind the C ABI (include/rpt/rpt.h rpt_denoise, rpt_denoise_variance, rpt_read_guides, rpt_denoise_params_default,
 * rpt_denoise_var_params_default, rpt_denoise_temporal, rpt_temporal_reset, rpt_temporal_params_default) and its host builds (rpt_debug.h rpt_debug_denoise_host,
 * rpt_debug_denoise_variance_host, rpt_debug_denoise_temporal_host, rpt_debug_firefly_host): the guide buffers of a context — built with the one-ray-per-lane nearest-hit walk the debug hook launches
 * (rpt_launch_trace_debug: LDS or global variant per scene, no new walk instantiated) and a small shading kernel — and the passes of k_denoise.h.
 */
#include <cstring>
#include <vector>

#include "rpt_ctx.h"
#include "k_denoise.h"
#include "k_guides_glass.h"
#include "k_adaptive.h"
#include "k_temporal.h"
#include "k_firefly.h"

namespace {

/* csrc/k_denoise.h; chosen on converged images of the shipped scenes: profiles/r11_denoise_quality.txt */
constexpr rpt_denoise_params DN_DEFAULTS = {2u, 0u, 1.0f, 2.0f, 1u, {0u, 0u, 0u}};

/* the grid of profiles/r14_denoise_variance_quality.txt (tools/denoise_probe.py --quality-variance).  The firefly clamp ships OFF (clamp_scale 0): a call
 * that does not ask for it returns what it returned before the fields existed.  clamp_radius is that of the lowest summed ratio of
 * profiles/r16_firefly_quality.txt (--quality-firefly), which a caller turns on with clamp_scale = 2 */
constexpr rpt_denoise_var_params DN_VAR_DEFAULTS = {DN_DEFAULTS, 0.0f, 0.0f, 0.0f, 1u};

/* the grid of profiles/r15_temporal_quality.txt (tools/denoise_probe.py --quality-temporal): with a history the variance term pays, so it is on here */
/* (the clamp off, as above; on the eight-view path the lowest summed ratio of profiles/r16_firefly_quality.txt is at this clamp_radius, 3, with clamp_scale = 1 —
 * not the 2 that goes with DN_VAR_DEFAULTS' radius 1) */
constexpr rpt_temporal_params TP_DEFAULTS = {{DN_DEFAULTS, 32.0f, 0.0f, 0.0f, 3u}, 8.0f, 0.5f, 0.5f, {0u, 0u, 0u, 0u, 0u}};

int check_params(const rpt_denoise_params &p, uint32_t tonemap_op, std::string &error) {
    if (p.iterations > RPT_DN_MAX_ITERATIONS) { error = "rpt_denoise: iterations must be 0..6"; return RPT_EINVAL; }
    if (p.normal_power_log2 > RPT_DN_MAX_NORMAL_POWER_LOG2) { error = "rpt_denoise: normal_power_log2 must be 0..10"; return RPT_EINVAL; }
    if (!rptm::finiter(p.sigma_color) || !rptm::finiter(p.sigma_plane) || p.sigma_color < 0.0f || p.sigma_plane < 0.0f) {
        error = "rpt_denoise: sigma_color and sigma_plane must be finite and >= 0";
        return RPT_EINVAL;
    }
    if (tonemap_op > 6u) { error = "tonemap operator must be 0..6"; return RPT_EINVAL; }
    return RPT_OK;
}

int check_var_params(const rpt_denoise_var_params &p, uint32_t tonemap_op, std::string &error) {
    RPT_TRY(check_params(p.base, tonemap_op, error));
    if (!(p.sigma_variance >= 0.0f)) { error = "rpt_denoise_variance: sigma_variance must be >= 0 (+inf allowed)"; return RPT_EINVAL; }
    if (!rptm::finiter(p.clamp_scale) || p.clamp_scale < 0.0f) { error = "rpt_denoise_variance: clamp_scale must be finite and >= 0"; return RPT_EINVAL; }
    if (p.clamp_scale == 0.0f) return RPT_OK;            /* the clamp is off: the other two words are not read */
    if (!rptm::finiter(p.clamp_floor) || p.clamp_floor < 0.0f) { error = "rpt_denoise_variance: clamp_floor must be finite and >= 0"; return RPT_EINVAL; }
    if (p.clamp_radius < 1u || p.clamp_radius > RPT_FF_MAX_RADIUS) { error = "rpt_denoise_variance: clamp_radius must be 1..3"; return RPT_EINVAL; }
    return RPT_OK;
}

int check_temporal_params(const rpt_temporal_params &p, uint32_t tonemap_op, std::string &error) {
    RPT_TRY(check_var_params(p.filter, tonemap_op, error));
    if (!(p.max_history >= 0.0f) || !(p.plane_max >= 0.0f)) { error = "rpt_denoise_temporal: max_history and plane_max must be >= 0 (+inf allowed)"; return RPT_EINVAL; }
    if (!(p.normal_min >= -1.0f && p.normal_min <= 1.0f)) { error = "rpt_denoise_temporal: normal_min must be in [-1, 1]"; return RPT_EINVAL; }
    return RPT_OK;
}

/* The plane term of the filters is the pixel footprint per unit depth, 2 / W (k_denoise.h DnPass::plane_scale), under a lens 2 tan_half_fov / W: the factor
 * enters through the parameter — sigma_plane * tan_half_fov, one f32 product on the host, the identity at 1.0f — so it reaches the device passes and the
 * host builds (rpt_debug_denoise_host, ..._variance_host: handed that sigma_plane) by the one route every parameter takes, dn_pass. */
float lens_sigma_plane(const rpt_ctx *c, float sigma_plane) { return sigma_plane * c->lens.tan_half_fov; }

/* buffers + events for the current configuration (first use, or the first use after a resize released them) */
int ensure_buffers(rpt_ctx *c) {
    DenoiseState &d = c->dn;
    const uint32_t W = c->cfg.c.width, H = c->cfg.c.height;
    const size_t n = (size_t)W * H;
    if (n > ((size_t)1 << 28)) { c->error = "rpt_denoise: images of more than 2^28 pixels are not supported"; return RPT_EINVAL; }
    for (hipEvent_t &e : d.ev)
        if (!e) HIP_TRY(c, hipEventCreate(&e));
    if (d.width == W && d.height == H && d.g0.p) return RPT_OK;
    rpt_denoise_release(c, false);
    std::vector<uint32_t> order;
    rpt_build_pixel_order(W, H, 0u, 1u, order);
    if (order.size() != n) { c->error = "rpt_denoise: internal error (tile order does not cover the image)"; return RPT_EHIP; }
    HIP_TRY(c, d.order.from_host(order.data(), n));
    HIP_TRY(c, d.g0.alloc(n)); HIP_TRY(c, d.g1.alloc(n)); HIP_TRY(c, d.albedo.alloc(n));
    HIP_TRY(c, d.ping.alloc(n)); HIP_TRY(c, d.pong.alloc(n)); HIP_TRY(c, d.rgb.alloc(3 * n));
    d.width = W; d.height = H;
    d.guides_valid = false;
    return RPT_OK;
}

/* rpt_set_guides_through_glass: the guides of a context whose setting is above 0 and some of whose records are Glass (k_guides_glass.h) — rounds of one walk
 * of the rays still inside glass and one step kernel, the survivors compacted in ascending order between them.  One 16-byte read per round sizes the next
 * launch; a round with no ray launches nothing.  The caller has waited for the batches. */
template <bool TEXTURED>
int build_guides_through_glass(rpt_ctx *c) {
    DenoiseState &d = c->dn;
    const uint32_t n = d.width * d.height, K = d.through_glass, blocks = rpt_blocks(n);
    const size_t vec = Arena::pad(3 * (size_t)n * sizeof(float)), word = Arena::pad((size_t)n * sizeof(uint32_t));
    Arena rays;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{c->stream};      /* (destroyed before the arena: no exit frees rays a kernel still reads) */
    HIP_TRY(c, rays.reserve(6 * vec + 6 * word + Arena::pad((size_t)n * sizeof(float4)) + Arena::pad(n) + 2 * Arena::pad((size_t)blocks * sizeof(uint32_t)) + Arena::pad(sizeof(GgResult))));
    float *origins0 = rays.take<float>(3 * (size_t)n), *dirs0 = rays.take<float>(3 * (size_t)n);                    /* the centre rays: round 0, and every position */
    float *next_o = rays.take<float>(3 * (size_t)n), *next_d = rays.take<float>(3 * (size_t)n);                     /* a round's rays that go on, at their own index */
    float *cur_o = rays.take<float>(3 * (size_t)n), *cur_d = rays.take<float>(3 * (size_t)n);                       /* ... compacted: the next round's rays */
    float *hit_t = rays.take<float>(n);
    uint32_t *hit_tri = rays.take<uint32_t>(n), *hit_flags = rays.take<uint32_t>(n), *next_slot = rays.take<uint32_t>(n), *cur_slot = rays.take<uint32_t>(n);
    uint32_t *interfaces = rays.take<uint32_t>(n);
    float4 *chain = rays.take<float4>(n);
    uint8_t *flags = rays.take<uint8_t>(n);
    uint32_t *wg_count = rays.take<uint32_t>(blocks), *wg_offset = rays.take<uint32_t>(blocks);
    GgResult *res = rays.take<GgResult>(1);
    const GgScene gs{c->scene.tri_geom, c->scene.tri_shade, c->scene.tri_tangent, c->scene.materials, c->scene.mat_lite, reinterpret_cast<const uint32_t *>(c->scene.atlas.texels),
                     c->scene.atlas.width, c->scene.atlas.height};
    const uint4 *models = reinterpret_cast<const uint4 *>(c->material_models.p);
    const GgNext next{next_o, next_d, next_slot, chain, interfaces, flags, wg_count};
    hipStream_t s = c->stream;
    d.info = rpt_guides_info{};
    GgResult got{};
    HIP_TRY(c, hipEventRecord(d.ev[0], s));
    HIP_TRY(c, hipMemsetAsync(res, 0, sizeof(GgResult), s));
    if (rpt_lens_active(c)) rpt_launch_guide_rays_lens(c, d.order.p, n, origins0, dirs0);      /* (rpt_set_camera_lens: pixel centre through the lens centre, with its field of view) */
    else k_dn_camera_rays<<<blocks, RPT_BLOCK, 0, s>>>(c->cfg, d.order.p, n, origins0, dirs0);
    uint32_t n_cur = n;
    for (uint32_t round = 0; round <= K && n_cur != 0u; ++round) {        /* (a ray of round r has crossed r interfaces: round K ends every chain) */
        const GgRays in{round ? cur_o : origins0, round ? cur_d : dirs0, round ? cur_slot : nullptr, hit_t, hit_tri, hit_flags};
        rpt_launch_trace_debug(c, 0, n_cur, in.origins, in.dirs, nullptr, hit_t, hit_tri, hit_flags);
        k_dn_glass_step<TEXTURED><<<rpt_blocks(n_cur), RPT_BLOCK, 0, s>>>(gs, models, K, round == 0u ? 1u : 0u, d.width, d.order.p, n_cur, in, origins0, dirs0, next, d.g0.p, d.g1.p,
                                                                         d.albedo.p, res);
        d.info.rays[round] = n_cur;
        d.info.rounds = round + 1u;
        if (round == K) break;
        k_dn_glass_scan<<<1, RPT_BLOCK, 0, s>>>(wg_count, rpt_blocks(n_cur), wg_offset, res);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&got, res, sizeof got, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        const uint32_t n_next = got.n_active <= n_cur ? got.n_active : n_cur;
        if (n_next != 0u) k_dn_glass_scatter<<<rpt_blocks(n_cur), RPT_BLOCK, 0, s>>>(n_cur, flags, wg_offset, n_next, next_o, next_d, next_slot, cur_o, cur_d, cur_slot);
        n_cur = n_next;
    }
    HIP_TRY(c, hipEventRecord(d.ev[1], s));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(&got, res, sizeof got, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));             /* (before the rays and the chains are freed) */
    d.info.pixels_through_glass = got.crossed;
    d.info.pixels_exhausted = got.exhausted;
    return RPT_OK;
}

/* the guides of (scene, configuration, setting), on the context's stream; *rebuilt = they were stale.  The rays and their hits live for this call only. */
int ensure_guides(rpt_ctx *c, bool *rebuilt) {
    DenoiseState &d = c->dn;
    *rebuilt = false;
    RPT_TRY(ensure_buffers(c));
    if (d.guides_valid) return RPT_OK;
    RPT_TRY(rpt_wait(c));                            /* the walk shares the context's stream (and LDS) with the batches */
    const uint32_t n = d.width * d.height;
    bool some_glass = false;
    for (const rpt_material_model &m : c->material_models_host) some_glass = some_glass || m.model == RPT_MODEL_GLASS;
    if (d.through_glass != 0u && some_glass) {       /* otherwise: exactly the launches below, as before the setting existed */
        RPT_TRY(c->scene.textured ? build_guides_through_glass<true>(c) : build_guides_through_glass<false>(c));
        d.guides_valid = true;
        *rebuilt = true;
        return RPT_OK;
    }
    d.info = rpt_guides_info{};
    d.info.rounds = 1u;
    d.info.rays[0] = n;
    Arena rays;
    HIP_TRY(c, rays.reserve(2 * Arena::pad(3 * (size_t)n * sizeof(float)) + 3 * Arena::pad((size_t)n * sizeof(uint32_t))));
    float *origins = rays.take<float>(3 * (size_t)n), *dirs = rays.take<float>(3 * (size_t)n), *hit_t = rays.take<float>(n);
    uint32_t *hit_tri = rays.take<uint32_t>(n), *hit_flags = rays.take<uint32_t>(n);
    hipStream_t s = c->stream;
    HIP_TRY(c, hipEventRecord(d.ev[0], s));
    if (rpt_lens_active(c)) rpt_launch_guide_rays_lens(c, d.order.p, n, origins, dirs);
    else k_dn_camera_rays<<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(c->cfg, d.order.p, n, origins, dirs);
    rpt_launch_trace_debug(c, 0, n, origins, dirs, nullptr, hit_t, hit_tri, hit_flags);
    if (c->scene.textured) k_dn_shade_guides<true><<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(c->scene, d.width, d.order.p, n, origins, dirs, hit_t, hit_tri, hit_flags, d.g0.p, d.g1.p, d.albedo.p);
    else k_dn_shade_guides<false><<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(c->scene, d.width, d.order.p, n, origins, dirs, hit_t, hit_tri, hit_flags, d.g0.p, d.g1.p, d.albedo.p);
    HIP_TRY(c, hipEventRecord(d.ev[1], s));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(s));             /* (before the rays are freed) */
    d.guides_valid = true;
    *rebuilt = true;
    return RPT_OK;
}

/* k_dn_prepare while the counts are non-uniform: every pixel's sum by its own count (k_adaptive.h mean_own) */
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_prepare_own(const float4 *sums, const uint32_t *order, uint32_t n, uint32_t width, const float4 *albedo /* null: no demodulation */, float4 *out) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    size_t at = i;
    if (order) at = rpt_pixel_index(order[i], width);
    F3 c = mean_own(sums[i]);
    if (albedo) c = dn_demodulate(c, xyz4(albedo[at]));
    out[at] = make_float4(c.x, c.y, c.z, 0.0f);
}

void launch_pass(hipStream_t s, const DnPass &ps, bool last, const float4 *src, const DenoiseState &d, float4 *dst, uint32_t demodulated, uint32_t tonemap_op) {
    const dim3 grid((ps.width + 63u) / 64u, (ps.height + 3u) / 4u);
    if (last) k_dn_pass<true><<<grid, 256, 0, s>>>(ps, src, d.g0.p, d.g1.p, dst, d.albedo.p, demodulated, tonemap_op, d.rgb.p);
    else k_dn_pass<false><<<grid, 256, 0, s>>>(ps, src, d.g0.p, d.g1.p, dst, d.albedo.p, demodulated, tonemap_op, d.rgb.p);
}

/* pre-pass: k_dn_prepare / k_dn_prepare_own (OWN: every pixel by its own .w) with the variance of the mean in the .w lane.  `order` != null: element i of
 * `sums` is pixel order[i]; the moments are in that order too (the context's record, beside its accumulator) unless moments_row_major (a caller's image) */
template <bool OWN>
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_prepare_var(const float4 *sums, const float4 *moments, const uint32_t *order, uint32_t moments_row_major, uint32_t n, uint32_t width,
                                                              float sample_count, const float4 *albedo /* null: no demodulation */, float4 *out) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    size_t at = i;
    if (order) at = rpt_pixel_index(order[i], width);
    const float4 a = sums[i];
    F3 c = OWN ? mean_own(a) : f3(a.x / sample_count, a.y / sample_count, a.z / sample_count);
    F3 al = f3s(1.0f);
    if (albedo) { al = xyz4(albedo[at]); c = dn_demodulate(c, al); }
    const float v = dn_prepare_variance(moments[moments_row_major ? at : (size_t)i], albedo != nullptr, al);
    out[at] = make_float4(c.x, c.y, c.z, v);
}

void launch_pass_var(hipStream_t s, const DnPass &ps, float sigma_variance, bool last, const float4 *src, const DenoiseState &d, float4 *dst, uint32_t demodulated, uint32_t tonemap_op) {
    const dim3 grid((ps.width + 63u) / 64u, (ps.height + 3u) / 4u);
    if (last) k_dn_pass_var<true><<<grid, 256, 0, s>>>(ps, sigma_variance, src, d.g0.p, d.g1.p, dst, d.albedo.p, demodulated, tonemap_op, d.rgb.p, d.variance.p);
    else k_dn_pass_var<false><<<grid, 256, 0, s>>>(ps, sigma_variance, src, d.g0.p, d.g1.p, dst, d.albedo.p, demodulated, tonemap_op, d.rgb.p, d.variance.p);
}

/* the image a call filters: the context's accumulator (tile-major, `order` = its pixels) or the last gather's (row-major, on the gather's stream) */
struct DnSource {
    const float4 *sums = nullptr;
    const uint32_t *order = nullptr;
    uint32_t samples = 0;
    bool own_counts = false;             /* counts are non-uniform: every pixel by its own accum.w */
    hipStream_t stream = nullptr;
};
int open_source(rpt_ctx *c, uint32_t source, DnSource *out) {
    if (source != RPT_DENOISE_ACCUM && source != RPT_DENOISE_GATHERED) { c->error = "rpt_denoise: source must be RPT_DENOISE_ACCUM or RPT_DENOISE_GATHERED"; return RPT_EINVAL; }
    if (!c->has_scene || !c->has_config || !c->has_state) { c->error = "rpt_denoise: needs a scene and a configuration"; return RPT_EINVAL; }
    HIP_TRY(c, hipSetDevice(c->device));
    DnSource src;
    src.stream = c->stream;
    if (source == RPT_DENOISE_ACCUM) {
        if (c->world != 1u) { c->error = "rpt_denoise: RPT_DENOISE_ACCUM needs a partition of one rank (this context is one of " + std::to_string(c->world) + "): gather, then RPT_DENOISE_GATHERED on rank 0"; return RPT_EINVAL; }
        RPT_TRY(rpt_wait(c));
        src.sums = c->accum.p; src.order = c->pixel_xy.p; src.samples = c->samples; src.own_counts = c->counts_nonuniform;
    } else {
        RPT_TRY(rpt_comm_gathered_image(c, &src.sums, &src.samples, &src.own_counts, &src.stream));
    }
    if (src.samples == 0u && !src.own_counts) { c->error = "rpt_denoise: the image has zero samples"; return RPT_EINVAL; }
    *out = src;
    return RPT_OK;
}

/* the moments a call filters by: the context's own record (beside its accumulator, in its order) or the caller's row-major image, uploaded for this call
 * (the previous call's kernels have drained: every call is synchronous on return).  `who`: the entry point, for the error text. */
int check_moments_source(rpt_ctx *c, uint32_t source, const float *moments_xyzw, const char *who) {
    if (moments_xyzw) return RPT_OK;
    if (source == RPT_DENOISE_GATHERED && rpt_comm_gather_moments_on(c)) {      /* the gathered record, once a gather has carried it (open_moments takes it) */
        const float4 *record = nullptr;
        return rpt_comm_gathered_moments(c, who, &record);
    }
    /* the context's own record: it lies beside the accumulator, and only there */
    if (source == RPT_DENOISE_GATHERED) { c->error = std::string(who) + ": moments are not part of the gather: RPT_DENOISE_GATHERED needs a moments image (rpt_read_moments / rpt_multi_read_moments)"; return RPT_EINVAL; }
    if (!c->moments_on) { c->error = std::string(who) + ": moments are off (rpt_set_moments(ctx, 1) first, or pass a moments image)"; return RPT_EINVAL; }
    return RPT_OK;
}
int open_moments(rpt_ctx *c, uint32_t source, const float *moments_xyzw, uint32_t n, const char *who, const float4 **out, uint32_t *row_major_out) {
    DenoiseState &d = c->dn;
    if (d.variance.n != n) HIP_TRY(c, d.variance.alloc(n));
    *out = c->moments.p;
    *row_major_out = moments_xyzw || source == RPT_DENOISE_GATHERED ? 1u : 0u;
    if (!moments_xyzw && source == RPT_DENOISE_GATHERED) return rpt_comm_gathered_moments(c, who, out);      /* (row-major, on the device, on the gather's stream) */
    if (moments_xyzw) {
        if (d.moments_in.n != n) HIP_TRY(c, d.moments_in.alloc(n));
        HIP_TRY(c, hipMemcpy(d.moments_in.p, moments_xyzw, (size_t)n * sizeof(float4), hipMemcpyHostToDevice));
        *out = d.moments_in.p;
    } else if (c->moments.n != n) {      /* (one rank owns every pixel: checked by open_source) */
        c->error = std::string(who) + ": internal error (the moments record does not cover the image)";
        return RPT_EHIP;
    }
    return RPT_OK;
}

/* the passes of the variance-guided filter over the prepared image in d.ping, into d.rgb and d.variance (iterations == 0: resolve only) */
void launch_var_passes(hipStream_t s, DenoiseState &d, const rpt_denoise_var_params &vp, bool demodulated, uint32_t tonemap_op) {
    const rpt_denoise_params &p = vp.base;
    const uint32_t W = d.width, H = d.height, n = W * H;
    if (p.iterations == 0u) {
        k_dn_resolve<<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(d.ping.p, n, tonemap_op, d.rgb.p);
        k_dn_variance_plane<<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(d.ping.p, n, d.variance.p);
    }
    float4 *src = d.ping.p, *dst = d.pong.p;
    for (uint32_t i = 0; i < p.iterations; ++i) {
        const DnPass ps = dn_pass(W, H, i, p.normal_power_log2, p.sigma_color, p.sigma_plane);
        launch_pass_var(s, ps, vp.sigma_variance, i + 1u == p.iterations, src, d, dst, demodulated ? 1u : 0u, tonemap_op);
        std::swap(src, dst);
    }
}

/* the host build of those passes: ping holds the prepared (e | v) */
void host_var_passes(uint32_t width, uint32_t height, const rpt_denoise_var_params &vp, bool demodulated, uint32_t tonemap_op, std::vector<float4> &ping, const std::vector<float4> &g0,
                     const std::vector<float4> &g1, const std::vector<float4> &a, float *out_rgb, float *out_variance) {
    const rpt_denoise_params &p = vp.base;
    const size_t n = (size_t)width * height;
    std::vector<float4> pong(n);
    std::vector<float4> *src = &ping, *dst = &pong;
    for (uint32_t i = 0; i < p.iterations; ++i) {
        const DnPass ps = dn_pass(width, height, i, p.normal_power_log2, p.sigma_color, p.sigma_plane);
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                const DnVarOut o = dn_filter_pixel_var(ps, vp.sigma_variance, src->data(), g0.data(), g1.data(), x, y);
                (*dst)[(size_t)y * width + x] = make_float4(o.e.x, o.e.y, o.e.z, o.v);
            }
        std::swap(src, dst);
    }
    for (size_t i = 0; i < n; ++i) {
        const float4 e = (*src)[i];
        const F3 c = dn_finish_pixel(f3(e.x, e.y, e.z), f3(a[i].x, a[i].y, a[i].z), demodulated, tonemap_op);
        out_rgb[3 * i] = c.x; out_rgb[3 * i + 1] = c.y; out_rgb[3 * i + 2] = c.z;
        if (out_variance) out_variance[i] = e.w;
    }
}

void fill_report(const DenoiseState &d, bool rebuilt, unsigned long long clamped, rpt_denoise_report *report) {
    float ms = 0.0f;
    *report = rpt_denoise_report{};
    report->pixels_clamped = (uint32_t)clamped;          /* (an image has at most 2^28 pixels) */
    if (hipEventElapsedTime(&ms, d.ev[2], d.ev[3]) == hipSuccess) report->device_ms = ms;
    if (rebuilt && hipEventElapsedTime(&ms, d.ev[0], d.ev[1]) == hipSuccess) report->guides_ms = ms;
    report->guides_rebuilt = rebuilt ? 1u : 0u;
}

/* the element of the context's tile-major records that is row-major pixel i, cached on the context (`order` == null — a gathered image — needs none) */
int ensure_inverse(rpt_ctx *c, const uint32_t *order, uint32_t W, uint32_t n, const char *who) {
    DenoiseState &d = c->dn;
    if (!order || d.inverse.n == n) return RPT_OK;       /* (one rank owns every pixel: the context's order is the whole image's) */
    if (c->pixel_xy_host.size() != n) { c->error = std::string(who) + ": internal error (the pixel order does not cover the image)"; return RPT_EHIP; }
    std::vector<uint32_t> inverse(n);
    for (uint32_t i = 0; i < n; ++i) inverse[rpt_pixel_index(c->pixel_xy_host[i], W)] = i;
    HIP_TRY(c, d.inverse.from_host(inverse.data(), n));
    return RPT_OK;
}

/* the firefly clamp of a call (k_firefly.h): its parameters and the images its window reads; the context's own record is tile-major, a caller's row-major */
FfView ff_view(const DenoiseState &d, const rpt_denoise_var_params &vp, bool demodulated, const float4 *moments, bool moments_tile_major) {
    return FfView{d.width, d.height, vp.clamp_radius, demodulated ? 1u : 0u, vp.clamp_scale, vp.clamp_floor, moments, moments_tile_major ? d.inverse.p : nullptr, d.g1.p, d.albedo.p};
}
int ensure_clamp_counter(rpt_ctx *c) {
    if (!c->dn.clamped.p) HIP_TRY(c, c->dn.clamped.alloc(1));
    return RPT_OK;
}

/* the two cameras of a call into its TpView: the current position, and — prev_ro != null — the previous view's, with the bit-for-bit comparison */
void tp_set_cameras(TpView &vw, const float *ro_cur, const float *euler_cur, const float *ro_prev, const float *euler_prev) {
    memcpy(vw.ro_cur, ro_cur, sizeof vw.ro_cur);
    if (!ro_prev) return;
    vw.has_history = 1u;
    memcpy(vw.ro_prev, ro_prev, sizeof vw.ro_prev);
    memcpy(vw.euler_prev, euler_prev, sizeof vw.euler_prev);
    vw.identity = memcmp(ro_cur, ro_prev, sizeof vw.ro_cur) == 0 && memcmp(euler_cur, euler_prev, sizeof vw.euler_prev) == 0 ? 1u : 0u;
}

}  // namespace

void rpt_denoise_release(rpt_ctx *c, bool events_too) {
    DenoiseState &d = c->dn;
    d.g0.release(); d.g1.release(); d.albedo.release(); d.ping.release(); d.pong.release(); d.rgb.release(); d.order.release(); d.variance.release(); d.moments_in.release();
    if (d.last.valid || d.previous.valid) d.history_dropped = true;      /* (a resize: the next rpt_denoise_temporal reports it) */
    d.last.release(); d.previous.release(); d.history_t.release(); d.inverse.release(); d.with_history.release(); d.clamped.release();
    d.width = d.height = 0;
    d.guides_valid = false;
    if (events_too)
        for (hipEvent_t &e : d.ev)
            if (e) { (void)hipEventDestroy(e); e = nullptr; }
}

extern "C" {

void rpt_denoise_params_default(rpt_denoise_params *out) {
    if (out) *out = DN_DEFAULTS;
}

int rpt_denoise(rpt_ctx *c, uint32_t source, const rpt_denoise_params *params, uint32_t tonemap_op, float *out_rgb, rpt_denoise_report *report) {
    if (!c || !out_rgb) return RPT_EINVAL;
    rpt_denoise_params p = params ? *params : DN_DEFAULTS;
    RPT_TRY(check_params(p, tonemap_op, c->error));
    p.sigma_plane = lens_sigma_plane(c, p.sigma_plane);
    DnSource in;
    RPT_TRY(open_source(c, source, &in));
    const float4 *sums = in.sums;
    const uint32_t *order = in.order;
    const uint32_t samples = in.samples;
    const bool own_counts = in.own_counts;
    hipStream_t s = in.stream;
    bool rebuilt = false;
    RPT_TRY(ensure_guides(c, &rebuilt));
    DenoiseState &d = c->dn;
    const uint32_t W = d.width, H = d.height, n = W * H;
    const bool demodulated = p.iterations != 0u && p.demodulate != 0u;
    HIP_TRY(c, hipEventRecord(d.ev[2], s));
    if (own_counts) k_dn_prepare_own<<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(sums, order, n, W, demodulated ? d.albedo.p : nullptr, d.ping.p);
    else k_dn_prepare<<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(sums, order, n, W, (float)samples, demodulated ? d.albedo.p : nullptr, d.ping.p);
    if (p.iterations == 0u) k_dn_resolve<<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(d.ping.p, n, tonemap_op, d.rgb.p);
    float4 *src = d.ping.p, *dst = d.pong.p;
    for (uint32_t i = 0; i < p.iterations; ++i) {
        const DnPass ps = dn_pass(W, H, i, p.normal_power_log2, p.sigma_color, p.sigma_plane);
        launch_pass(s, ps, i + 1u == p.iterations, src, d, dst, demodulated ? 1u : 0u, tonemap_op);
        std::swap(src, dst);
    }
    HIP_TRY(c, hipEventRecord(d.ev[3], s));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out_rgb, d.rgb.p, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (report) {
        float ms = 0.0f;
        *report = rpt_denoise_report{};
        if (hipEventElapsedTime(&ms, d.ev[2], d.ev[3]) == hipSuccess) report->device_ms = ms;
        if (rebuilt && hipEventElapsedTime(&ms, d.ev[0], d.ev[1]) == hipSuccess) report->guides_ms = ms;
        report->guides_rebuilt = rebuilt ? 1u : 0u;
    }
    return RPT_OK;
}

void rpt_denoise_var_params_default(rpt_denoise_var_params *out) {
    if (out) *out = DN_VAR_DEFAULTS;
}

int rpt_denoise_variance(rpt_ctx *c, uint32_t source, const float *moments_xyzw, const rpt_denoise_var_params *params, uint32_t tonemap_op, float *out_rgb, float *out_variance,
                         rpt_denoise_report *report) {
    if (!c) return RPT_EINVAL;
    if (!out_rgb) { c->error = "rpt_denoise_variance: out_rgb is null"; return RPT_EINVAL; }
    rpt_denoise_var_params vp = params ? *params : DN_VAR_DEFAULTS;
    const rpt_denoise_params &p = vp.base;
    RPT_TRY(check_var_params(vp, tonemap_op, c->error));
    vp.base.sigma_plane = lens_sigma_plane(c, vp.base.sigma_plane);
    RPT_TRY(check_moments_source(c, source, moments_xyzw, "rpt_denoise_variance"));
    DnSource in;
    RPT_TRY(open_source(c, source, &in));
    hipStream_t s = in.stream;
    bool rebuilt = false;
    RPT_TRY(ensure_guides(c, &rebuilt));
    DenoiseState &d = c->dn;
    const uint32_t W = d.width, H = d.height, n = W * H;
    const float4 *moments = nullptr;
    uint32_t row_major = 0u;
    RPT_TRY(open_moments(c, source, moments_xyzw, n, "rpt_denoise_variance", &moments, &row_major));
    const bool demodulated = p.iterations != 0u && p.demodulate != 0u;
    const float4 *albedo = demodulated ? d.albedo.p : nullptr;
    const bool clamp = vp.clamp_scale != 0.0f;
    if (clamp) {
        RPT_TRY(ensure_inverse(c, in.order, W, n, "rpt_denoise_variance"));
        RPT_TRY(ensure_clamp_counter(c));
    }
    HIP_TRY(c, hipEventRecord(d.ev[2], s));
    if (clamp) {                                         /* k_dn_prepare_var_clamp in place of k_dn_prepare_var */
        const FfView fv = ff_view(d, vp, demodulated, moments, in.order && !row_major);
        const uint32_t *inverse = in.order ? d.inverse.p : nullptr;
        const dim3 grid((W + 63u) / 64u, (H + 3u) / 4u);
        HIP_TRY(c, hipMemsetAsync(d.clamped.p, 0, sizeof(unsigned long long), s));
        if (in.own_counts) k_dn_prepare_var_clamp<true><<<grid, 256, 0, s>>>(fv, in.sums, inverse, 0.0f, d.ping.p, d.clamped.p);
        else k_dn_prepare_var_clamp<false><<<grid, 256, 0, s>>>(fv, in.sums, inverse, (float)in.samples, d.ping.p, d.clamped.p);
    } else if (in.own_counts) k_dn_prepare_var<true><<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(in.sums, moments, in.order, row_major, n, W, 0.0f, albedo, d.ping.p);
    else k_dn_prepare_var<false><<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(in.sums, moments, in.order, row_major, n, W, (float)in.samples, albedo, d.ping.p);
    launch_var_passes(s, d, vp, demodulated, tonemap_op);
    HIP_TRY(c, hipEventRecord(d.ev[3], s));
    HIP_TRY(c, hipGetLastError());
    unsigned long long clamped = 0ull;
    HIP_TRY(c, hipMemcpyAsync(out_rgb, d.rgb.p, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (out_variance) HIP_TRY(c, hipMemcpyAsync(out_variance, d.variance.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (clamp) HIP_TRY(c, hipMemcpyAsync(&clamped, d.clamped.p, sizeof clamped, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (report) fill_report(d, rebuilt, clamped, report);
    return RPT_OK;
}

void rpt_temporal_params_default(rpt_temporal_params *out) {
    if (out) *out = TP_DEFAULTS;
}

int rpt_temporal_reset(rpt_ctx *c) {
    if (!c) return RPT_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    DenoiseState &d = c->dn;
    d.last.release(); d.previous.release(); d.history_t.release(); d.inverse.release(); d.with_history.release();
    d.history_dropped = false;
    return RPT_OK;
}

int rpt_denoise_temporal(rpt_ctx *c, uint32_t source, const float *moments_xyzw, const rpt_temporal_params *params, uint32_t tonemap_op, float *out_rgb, float *out_variance,
                         float *out_history, rpt_temporal_report *report) {
    if (!c) return RPT_EINVAL;
    if (!out_rgb) { c->error = "rpt_denoise_temporal: out_rgb is null"; return RPT_EINVAL; }
    const rpt_temporal_params tp = params ? *params : TP_DEFAULTS;
    const rpt_denoise_params &p = tp.filter.base;
    RPT_TRY(check_temporal_params(tp, tonemap_op, c->error));
    if (c->lens.tan_half_fov != 1.0f) {      /* (an aperture alone: the projection is the lens centre's, the reference camera's) */
        c->error = "rpt_denoise_temporal: the camera lens has a field of view (tan_half_fov != 1): the reprojection is the inverse of the reference's camera; "
                   "rpt_denoise_variance filters the same image without history";
        return RPT_EINVAL;
    }
    RPT_TRY(check_moments_source(c, source, moments_xyzw, "rpt_denoise_temporal"));
    DnSource in;
    RPT_TRY(open_source(c, source, &in));
    hipStream_t s = in.stream;
    bool rebuilt = false;
    RPT_TRY(ensure_guides(c, &rebuilt));
    DenoiseState &d = c->dn;
    const uint32_t W = d.width, H = d.height, n = W * H;
    const float4 *moments = nullptr;
    uint32_t row_major = 0u;
    RPT_TRY(open_moments(c, source, moments_xyzw, n, "rpt_denoise_temporal", &moments, &row_major));
    const bool demodulated = p.iterations != 0u && p.demodulate != 0u;
    const float4 *albedo = demodulated ? d.albedo.p : nullptr;

    /* the slots: drop what no longer fits, promote once per accumulator epoch (a resize has freed them already) */
    uint32_t state = 0u;
    const bool units_differ = (d.last.valid && d.last.demodulated != demodulated) || (d.previous.valid && d.previous.demodulated != demodulated);
    if (d.history_dropped || ((d.last.valid || d.previous.valid) && (d.scene_changed || units_differ))) {
        d.last.release(); d.previous.release();
        state = 2u;
    }
    d.history_dropped = d.scene_changed = false;
    if (d.last.valid && d.last.epoch != c->accum_epoch) {
        std::swap(d.last, d.previous);
        d.last.valid = false;
    }
    if (d.previous.valid) state = 1u;
    TemporalSlot &last = d.last;
    if (last.h.n != n) { HIP_TRY(c, last.h.alloc(n)); HIP_TRY(c, last.g0.alloc(n)); HIP_TRY(c, last.g1.alloc(n)); HIP_TRY(c, last.mu.alloc(n)); }
    if (d.history_t.n != n) HIP_TRY(c, d.history_t.alloc(n));
    if (!d.with_history.p) HIP_TRY(c, d.with_history.alloc(1));
    RPT_TRY(ensure_inverse(c, in.order, W, n, "rpt_denoise_temporal"));
    const bool clamp = tp.filter.clamp_scale != 0.0f;
    if (clamp) RPT_TRY(ensure_clamp_counter(c));
    TpView vw = tp_view(W, H, tp.max_history, tp.normal_min, tp.plane_max);
    tp_set_cameras(vw, c->cfg.c.cam_position, c->cfg.euler, d.previous.valid ? d.previous.ro : nullptr, d.previous.euler);
    const TpPrev pv = d.previous.valid ? TpPrev{d.previous.h.p, d.previous.mu.p, d.previous.g0.p, d.previous.g1.p} : TpPrev{nullptr, nullptr, nullptr, nullptr};
    const uint32_t *inverse = in.order ? d.inverse.p : nullptr;
    const dim3 grid((W + 63u) / 64u, (H + 3u) / 4u);
    last.valid = false;
    HIP_TRY(c, hipEventRecord(d.ev[2], s));
    HIP_TRY(c, hipMemsetAsync(d.with_history.p, 0, sizeof(unsigned long long), s));
    if (clamp) {                                         /* k_dn_temporal_clamp in place of k_dn_temporal */
        const FfView fv = ff_view(d, tp.filter, demodulated, moments, in.order && !row_major);
        HIP_TRY(c, hipMemsetAsync(d.clamped.p, 0, sizeof(unsigned long long), s));
        if (in.own_counts) k_dn_temporal_clamp<true><<<grid, 256, 0, s>>>(fv, vw, pv, in.sums, inverse, 0.0f, d.g0.p, d.ping.p, last.h.p, last.mu.p, d.history_t.p, d.with_history.p, d.clamped.p);
        else k_dn_temporal_clamp<false><<<grid, 256, 0, s>>>(fv, vw, pv, in.sums, inverse, (float)in.samples, d.g0.p, d.ping.p, last.h.p, last.mu.p, d.history_t.p, d.with_history.p, d.clamped.p);
    } else if (in.own_counts) k_dn_temporal<true><<<grid, 256, 0, s>>>(vw, pv, in.sums, moments, inverse, row_major, 0.0f, d.g0.p, d.g1.p, albedo, d.ping.p, last.h.p, last.mu.p, d.history_t.p, d.with_history.p);
    else k_dn_temporal<false><<<grid, 256, 0, s>>>(vw, pv, in.sums, moments, inverse, row_major, (float)in.samples, d.g0.p, d.g1.p, albedo, d.ping.p, last.h.p, last.mu.p, d.history_t.p, d.with_history.p);
    HIP_TRY(c, hipMemcpyAsync(last.g0.p, d.g0.p, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(last.g1.p, d.g1.p, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, s));
    launch_var_passes(s, d, tp.filter, demodulated, tonemap_op);
    HIP_TRY(c, hipEventRecord(d.ev[3], s));
    HIP_TRY(c, hipGetLastError());
    unsigned long long with_history = 0ull, clamped = 0ull;
    HIP_TRY(c, hipMemcpyAsync(out_rgb, d.rgb.p, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (out_variance) HIP_TRY(c, hipMemcpyAsync(out_variance, d.variance.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (out_history) HIP_TRY(c, hipMemcpyAsync(out_history, d.history_t.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&with_history, d.with_history.p, sizeof with_history, hipMemcpyDeviceToHost, s));
    if (clamp) HIP_TRY(c, hipMemcpyAsync(&clamped, d.clamped.p, sizeof clamped, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    last.valid = true;
    last.epoch = c->accum_epoch;
    last.demodulated = demodulated;
    memcpy(last.ro, c->cfg.c.cam_position, sizeof last.ro);
    memcpy(last.euler, c->cfg.euler, sizeof last.euler);
    if (report) {
        *report = rpt_temporal_report{};
        fill_report(d, rebuilt, clamped, &report->base);
        report->pixels_with_history = with_history;
        report->history_state = state;
    }
    return RPT_OK;
}

int rpt_read_guides(rpt_ctx *c, float *albedo_rgb, float *normal_xyz, float *depth, float *position_xyz, uint32_t *kind) {
    if (!c) return RPT_EINVAL;
    if (!c->has_scene || !c->has_config || !c->has_state) { c->error = "rpt_read_guides: needs a scene and a configuration"; return RPT_EINVAL; }
    HIP_TRY(c, hipSetDevice(c->device));
    bool rebuilt = false;
    RPT_TRY(ensure_guides(c, &rebuilt));
    const DenoiseState &d = c->dn;
    const uint32_t n = d.width * d.height;
    const size_t rgb_bytes = Arena::pad(3 * (size_t)n * sizeof(float)), word_bytes = Arena::pad((size_t)n * sizeof(uint32_t));
    const size_t bytes = (albedo_rgb ? rgb_bytes : 0) + (normal_xyz ? rgb_bytes : 0) + (position_xyz ? rgb_bytes : 0) + (depth ? word_bytes : 0) + (kind ? word_bytes : 0);
    if (bytes == 0) return RPT_OK;                   /* nothing asked for: the guides are built, that is all */
    Arena planes;                                    /* only the planes the caller takes */
    HIP_TRY(c, planes.reserve(bytes));
    float *d_albedo = albedo_rgb ? planes.take<float>(3 * (size_t)n) : nullptr, *d_normal = normal_xyz ? planes.take<float>(3 * (size_t)n) : nullptr;
    float *d_position = position_xyz ? planes.take<float>(3 * (size_t)n) : nullptr, *d_depth = depth ? planes.take<float>(n) : nullptr;
    uint32_t *d_kind = kind ? planes.take<uint32_t>(n) : nullptr;
    k_dn_unpack_guides<<<rpt_blocks(n), RPT_BLOCK, 0, c->stream>>>(d.g0.p, d.g1.p, d.albedo.p, n, d_albedo, d_normal, d_depth, d_position, d_kind);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (albedo_rgb) HIP_TRY(c, hipMemcpy(albedo_rgb, d_albedo, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (normal_xyz) HIP_TRY(c, hipMemcpy(normal_xyz, d_normal, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (position_xyz) HIP_TRY(c, hipMemcpy(position_xyz, d_position, 3 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (depth) HIP_TRY(c, hipMemcpy(depth, d_depth, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    if (kind) HIP_TRY(c, hipMemcpy(kind, d_kind, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_set_guides_through_glass(rpt_ctx *c, uint32_t max_interfaces) {
    if (!c) return RPT_EINVAL;
    if (max_interfaces > RPT_GG_MAX_INTERFACES) { c->error = "rpt_set_guides_through_glass: max_interfaces must be 0..8"; return RPT_EINVAL; }
    if (c->dn.through_glass != max_interfaces) c->dn.guides_valid = false;
    c->dn.through_glass = max_interfaces;
    return RPT_OK;
}

int rpt_guides_through_glass(rpt_ctx *c, uint32_t *max_interfaces_out) {
    if (!c) return RPT_EINVAL;
    if (!max_interfaces_out) { c->error = "rpt_guides_through_glass: max_interfaces_out is null"; return RPT_EINVAL; }
    *max_interfaces_out = c->dn.through_glass;
    return RPT_OK;
}

int rpt_guides_info_get(rpt_ctx *c, rpt_guides_info *out) {
    if (!c) return RPT_EINVAL;
    if (!out) { c->error = "rpt_guides_info_get: out is null"; return RPT_EINVAL; }
    *out = c->dn.info;
    out->max_interfaces = c->dn.through_glass;
    return RPT_OK;
}

/* one step of the chain on the host: the loop k_dn_glass_step is, over the same RPT_HD function; the records of the triangle at hand as k_derive_triangles
 * (rpt_scene.hip) derives them */
int rpt_debug_glass_step_host(const rpt_per_vertex_data *vertices, size_t n_vertices, const rpt_triangle *indices, size_t n_triangles, const rpt_material_data *materials,
                              size_t n_materials, const uint8_t *atlas_rgba8, uint32_t atlas_w, uint32_t atlas_h, const rpt_material_model *models, uint32_t max_interfaces, size_t n,
                              float *origins_xyz, float *dirs_xyz, const float *hit_t, const uint32_t *hit_tri, const uint32_t *hit_flags, float *chain_albedo, float *chain_length,
                              uint32_t *chain_interfaces, uint8_t *active_out, uint32_t *kind_out, float *normal_out, float *albedo_out, uint8_t *exhausted_out) {
    if (!vertices || !indices || !materials || !origins_xyz || !dirs_xyz || !hit_t || !hit_tri || !hit_flags || !chain_albedo || !chain_length || !chain_interfaces || !active_out ||
        !kind_out || !normal_out || !albedo_out || !exhausted_out)
        return RPT_EINVAL;
    if (max_interfaces > RPT_GG_MAX_INTERFACES) { rpt_create_error() = "rpt_debug_glass_step_host: max_interfaces must be 0..8"; return RPT_EINVAL; }
    bool textured = false;
    std::vector<float4> lite(2 * n_materials);
    for (size_t i = 0; i < n_materials; ++i) {
        const rpt_material_data &m = materials[i];
        lite[2 * i + 0] = make_float4(m.emissive[0], m.emissive[1], m.emissive[2], m.roughness[0]);
        lite[2 * i + 1] = make_float4(m.albedo[0], m.albedo[1], m.albedo[2], m.metallic[0]);
        if (m.has_albedo_texture | m.has_metallic_texture | m.has_roughness_texture | m.has_normal_texture) textured = true;
    }
    if (textured && (!atlas_rgba8 || atlas_w == 0u || atlas_h == 0u)) { rpt_create_error() = "rpt_debug_glass_step_host: a material has a texture flag and there is no atlas"; return RPT_EINVAL; }
    static_assert(sizeof(rpt_material_data) == 6 * sizeof(float4) && sizeof(rpt_material_model) == sizeof(uint4), "the records are read as float4 / uint4");
    float4 geom[3], shade[4], tangent[3];
    const GgScene gs{geom, shade, tangent, reinterpret_cast<const float4 *>(materials), lite.data(), reinterpret_cast<const uint32_t *>(atlas_rgba8), atlas_w, atlas_h};
    for (size_t i = 0; i < n; ++i) {
        const bool is_hit = (hit_flags[i] & 1u) != 0u;
        if (is_hit) {
            if (hit_tri[i] >= n_triangles) { rpt_create_error() = "rpt_debug_glass_step_host: a triangle index is out of range"; return RPT_EINVAL; }
            const rpt_triangle &t = indices[hit_tri[i]];
            if (t.v0 >= n_vertices || t.v1 >= n_vertices || t.v2 >= n_vertices || t.material >= n_materials) { rpt_create_error() = "rpt_debug_glass_step_host: a vertex or material index is out of range"; return RPT_EINVAL; }
            const rpt_per_vertex_data &A = vertices[t.v0], &B = vertices[t.v1], &C = vertices[t.v2];
            const float *a = A.vertex, *b = B.vertex, *cc = C.vertex;
            const float e1x = b[0] - a[0], e1y = b[1] - a[1], e1z = b[2] - a[2];
            const float e2x = cc[0] - a[0], e2y = cc[1] - a[1], e2z = cc[2] - a[2];
            geom[0] = make_float4(a[0], a[1], a[2], (e1x * e1x + e1y * e1y) + e1z * e1z);
            geom[1] = make_float4(e1x, e1y, e1z, (e1x * e2x + e1y * e2y) + e1z * e2z);
            geom[2] = make_float4(e2x, e2y, e2z, (e2x * e2x + e2y * e2y) + e2z * e2z);
            shade[0] = make_float4(A.normal[0], A.normal[1], A.normal[2], A.uv0[0]);
            shade[1] = make_float4(B.normal[0], B.normal[1], B.normal[2], A.uv0[1]);
            shade[2] = make_float4(C.normal[0], C.normal[1], C.normal[2], rptm::u2f(t.material));
            shade[3] = make_float4(B.uv0[0], B.uv0[1], C.uv0[0], C.uv0[1]);
            tangent[0] = make_float4(A.tangent[0], A.tangent[1], A.tangent[2], A.tangent[3]);
            tangent[1] = make_float4(B.tangent[0], B.tangent[1], B.tangent[2], B.tangent[3]);
            tangent[2] = make_float4(C.tangent[0], C.tangent[1], C.tangent[2], C.tangent[3]);
        }
        float *o = origins_xyz + 3 * i, *dd = dirs_xyz + 3 * i, *ca = chain_albedo + 3 * i;
        const GgChain ch{f3(ca[0], ca[1], ca[2]), chain_length[i], chain_interfaces[i]};
        const uint4 *mo = reinterpret_cast<const uint4 *>(models);
        const GgStep s = textured ? dn_glass_step<true>(gs, mo, max_interfaces, f3(o[0], o[1], o[2]), f3(dd[0], dd[1], dd[2]), hit_t[i], 0u, is_hit, ch)
                                  : dn_glass_step<false>(gs, mo, max_interfaces, f3(o[0], o[1], o[2]), f3(dd[0], dd[1], dd[2]), hit_t[i], 0u, is_hit, ch);
        active_out[i] = s.final ? 0u : 1u;
        exhausted_out[i] = s.final && s.exhausted ? 1u : 0u;
        kind_out[i] = s.kind;
        normal_out[3 * i] = s.normal.x; normal_out[3 * i + 1] = s.normal.y; normal_out[3 * i + 2] = s.normal.z;
        albedo_out[3 * i] = s.albedo.x; albedo_out[3 * i + 1] = s.albedo.y; albedo_out[3 * i + 2] = s.albedo.z;
        o[0] = s.ro.x; o[1] = s.ro.y; o[2] = s.ro.z;
        dd[0] = s.rd.x; dd[1] = s.rd.y; dd[2] = s.rd.z;
        ca[0] = s.chain.A.x; ca[1] = s.chain.A.y; ca[2] = s.chain.A.z;
        chain_length[i] = s.chain.L;
        chain_interfaces[i] = s.chain.m;
    }
    return RPT_OK;
}

/* the filter on the host: the loop the kernels of k_denoise.h are, over the same RPT_HD functions */
int rpt_debug_denoise_host(uint32_t width, uint32_t height, const float *mean_rgb, const float *albedo, const float *normal, const float *position, const float *depth,
                           const uint32_t *kind, const rpt_denoise_params *params, uint32_t tonemap_op, float *out_rgb) {
    if (!mean_rgb || !albedo || !normal || !position || !depth || !kind || !out_rgb || width == 0u || height == 0u || width > 65535u || height > 65535u) return RPT_EINVAL;
    const rpt_denoise_params p = params ? *params : DN_DEFAULTS;
    std::string error;
    if (check_params(p, tonemap_op, error)) { rpt_create_error() = error; return RPT_EINVAL; }
    const size_t n = (size_t)width * height;
    const bool demodulated = p.iterations != 0u && p.demodulate != 0u;
    std::vector<float4> g0(n), g1(n), a(n), ping(n), pong(n);
    for (size_t i = 0; i < n; ++i) {
        g0[i] = make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], depth[i]);
        g1[i] = make_float4(position[3 * i], position[3 * i + 1], position[3 * i + 2], rptm::u2f(kind[i]));
        a[i] = make_float4(albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], 0.0f);
        F3 c = f3(mean_rgb[3 * i], mean_rgb[3 * i + 1], mean_rgb[3 * i + 2]);
        if (demodulated) c = dn_demodulate(c, f3(a[i].x, a[i].y, a[i].z));
        ping[i] = make_float4(c.x, c.y, c.z, 0.0f);
    }
    std::vector<float4> *src = &ping, *dst = &pong;
    for (uint32_t i = 0; i < p.iterations; ++i) {
        const DnPass ps = dn_pass(width, height, i, p.normal_power_log2, p.sigma_color, p.sigma_plane);
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                const F3 e = dn_filter_pixel(ps, src->data(), g0.data(), g1.data(), x, y);
                (*dst)[(size_t)y * width + x] = make_float4(e.x, e.y, e.z, 0.0f);
            }
        std::swap(src, dst);
    }
    for (size_t i = 0; i < n; ++i) {
        const float4 e = (*src)[i];
        const F3 c = dn_finish_pixel(f3(e.x, e.y, e.z), f3(a[i].x, a[i].y, a[i].z), demodulated, tonemap_op);
        out_rgb[3 * i] = c.x; out_rgb[3 * i + 1] = c.y; out_rgb[3 * i + 2] = c.z;
    }
    return RPT_OK;
}

/* the variance-guided filter on the host: the loop k_dn_prepare_var / k_dn_pass_var are, over the same RPT_HD functions */
int rpt_debug_denoise_variance_host(uint32_t width, uint32_t height, const float *mean_rgb, const float *albedo, const float *normal, const float *position, const float *depth,
                                    const uint32_t *kind, const float *moments_xyzw, const rpt_denoise_var_params *params, uint32_t tonemap_op, float *out_rgb, float *out_variance) {
    if (!mean_rgb || !albedo || !normal || !position || !depth || !kind || !moments_xyzw || !out_rgb || width == 0u || height == 0u || width > 65535u || height > 65535u) return RPT_EINVAL;
    const rpt_denoise_var_params vp = params ? *params : DN_VAR_DEFAULTS;
    const rpt_denoise_params &p = vp.base;
    std::string error;
    if (check_var_params(vp, tonemap_op, error)) { rpt_create_error() = error; return RPT_EINVAL; }
    const size_t n = (size_t)width * height;
    const bool demodulated = p.iterations != 0u && p.demodulate != 0u;
    std::vector<float4> g0(n), g1(n), a(n), ping(n), mo(n);
    for (size_t i = 0; i < n; ++i) {
        g0[i] = make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], depth[i]);
        g1[i] = make_float4(position[3 * i], position[3 * i + 1], position[3 * i + 2], rptm::u2f(kind[i]));
        a[i] = make_float4(albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], 0.0f);
        mo[i] = make_float4(moments_xyzw[4 * i], moments_xyzw[4 * i + 1], moments_xyzw[4 * i + 2], moments_xyzw[4 * i + 3]);
    }
    const bool clamp = vp.clamp_scale != 0.0f;
    const FfView fv{width, height, vp.clamp_radius, demodulated ? 1u : 0u, vp.clamp_scale, vp.clamp_floor, mo.data(), nullptr, g1.data(), a.data()};
    for (size_t i = 0; i < n; ++i) {
        const F3 al = f3(a[i].x, a[i].y, a[i].z);
        F3 c = f3(mean_rgb[3 * i], mean_rgb[3 * i + 1], mean_rgb[3 * i + 2]);
        float4 m = mo[i];
        if (clamp) {                                     /* (the hook is handed no count: the record's own) */
            const FfOut f = ff_pixel(fv, (uint32_t)(i % width), (uint32_t)(i / width), c, m.z, m);
            c = f.c; m = f.m;
        }
        if (demodulated) c = dn_demodulate(c, al);
        ping[i] = make_float4(c.x, c.y, c.z, dn_prepare_variance(m, demodulated, al));
    }
    host_var_passes(width, height, vp, demodulated, tonemap_op, ping, g0, g1, a, out_rgb, out_variance);
    return RPT_OK;
}

/* rpt_denoise_temporal on the host: the loop k_dn_temporal is, over the same RPT_HD function, then the passes above */
int rpt_debug_denoise_temporal_host(uint32_t width, uint32_t height, const float *mean_rgb, const float *albedo, const float *normal, const float *position, const float *depth,
                                    const uint32_t *kind, const float *moments_xyzw, const rpt_tracing_config *camera, const rpt_tracing_config *prev_camera, const float *prev_normal,
                                    const float *prev_position, const uint32_t *prev_kind, const float *prev_history, const rpt_temporal_params *params, uint32_t tonemap_op, float *out_rgb,
                                    float *out_variance, float *out_history, float *out_records, uint64_t *pixels_with_history_out) {
    if (!mean_rgb || !albedo || !normal || !position || !depth || !kind || !moments_xyzw || !camera || !out_rgb || width == 0u || height == 0u || width > 65535u || height > 65535u) return RPT_EINVAL;
    if (prev_camera && (!prev_normal || !prev_position || !prev_kind || !prev_history)) return RPT_EINVAL;
    const rpt_temporal_params tp = params ? *params : TP_DEFAULTS;
    const rpt_denoise_params &p = tp.filter.base;
    std::string error;
    if (check_temporal_params(tp, tonemap_op, error)) { rpt_create_error() = error; return RPT_EINVAL; }
    if (camera->width != width || camera->height != height || (prev_camera && (prev_camera->width != width || prev_camera->height != height))) {
        rpt_create_error() = "rpt_debug_denoise_temporal_host: a camera's width and height must be the image's";
        return RPT_EINVAL;
    }
    const size_t n = (size_t)width * height;
    const bool demodulated = p.iterations != 0u && p.demodulate != 0u;
    TpView vw = tp_view(width, height, tp.max_history, tp.normal_min, tp.plane_max);
    float euler_cur[9], euler_prev[9] = {};
    rpt_camera_matrix(camera->cam_rotation, euler_cur);
    if (prev_camera) rpt_camera_matrix(prev_camera->cam_rotation, euler_prev);
    tp_set_cameras(vw, camera->cam_position, euler_cur, prev_camera ? prev_camera->cam_position : nullptr, euler_prev);
    std::vector<float4> g0(n), g1(n), a(n), ping(n), mo(n), ph, pg0, pg1;
    std::vector<float2> pmu;
    if (prev_camera) {
        ph.resize(n); pg0.resize(n); pg1.resize(n); pmu.resize(n);
        for (size_t i = 0; i < n; ++i) {
            ph[i] = make_float4(prev_history[6 * i], prev_history[6 * i + 1], prev_history[6 * i + 2], prev_history[6 * i + 3]);
            pmu[i] = make_float2(prev_history[6 * i + 4], prev_history[6 * i + 5]);
            pg0[i] = make_float4(prev_normal[3 * i], prev_normal[3 * i + 1], prev_normal[3 * i + 2], 0.0f);      /* (a tap reads no depth) */
            pg1[i] = make_float4(prev_position[3 * i], prev_position[3 * i + 1], prev_position[3 * i + 2], rptm::u2f(prev_kind[i]));
        }
    }
    const TpPrev pv = TpPrev{ph.data(), pmu.data(), pg0.data(), pg1.data()};
    uint64_t with_history = 0;
    for (size_t i = 0; i < n; ++i) {
        g0[i] = make_float4(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], depth[i]);
        g1[i] = make_float4(position[3 * i], position[3 * i + 1], position[3 * i + 2], rptm::u2f(kind[i]));
        a[i] = make_float4(albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], 0.0f);
        mo[i] = make_float4(moments_xyzw[4 * i], moments_xyzw[4 * i + 1], moments_xyzw[4 * i + 2], moments_xyzw[4 * i + 3]);
    }
    const bool clamp = tp.filter.clamp_scale != 0.0f;
    const FfView fv{width, height, tp.filter.clamp_radius, demodulated ? 1u : 0u, tp.filter.clamp_scale, tp.filter.clamp_floor, mo.data(), nullptr, g1.data(), a.data()};
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            const F3 al = f3(a[i].x, a[i].y, a[i].z);
            F3 c = f3(mean_rgb[3 * i], mean_rgb[3 * i + 1], mean_rgb[3 * i + 2]);
            float4 m = mo[i];
            if (clamp) {                                 /* (the hook is handed no count: the record's own) */
                const FfOut f = ff_pixel(fv, x, y, c, m.z, m);
                c = f.c; m = f.m;
            }
            if (demodulated) c = dn_demodulate(c, al);
            const TpOut o = tp_pixel(vw, pv, x, y, c, m, g0[i], g1[i], demodulated, al);
            ping[i] = make_float4(o.e.x, o.e.y, o.e.z, o.v);
            if (out_history) out_history[i] = o.T;
            if (out_records) {
                float *r = out_records + 6 * i;
                r[0] = o.e.x; r[1] = o.e.y; r[2] = o.e.z; r[3] = o.N; r[4] = o.mu1; r[5] = o.mu2;
            }
            with_history += o.reused ? 1u : 0u;
        }
    if (pixels_with_history_out) *pixels_with_history_out = with_history;
    host_var_passes(width, height, tp.filter, demodulated, tonemap_op, ping, g0, g1, a, out_rgb, out_variance);
    return RPT_OK;
}

/* the firefly clamp on the host: the loop in front of k_dn_prepare_var_clamp / k_dn_temporal_clamp, over the same RPT_HD function */
int rpt_debug_firefly_host(uint32_t width, uint32_t height, const float *mean_rgb, const float *albedo, const uint32_t *kind, const float *moments_xyzw, const float *counts,
                           uint32_t samples, float clamp_scale, float clamp_floor, uint32_t clamp_radius, uint32_t demodulated, float *out_rgb, float *out_moments_xyzw, uint8_t *out_mask) {
    if (!mean_rgb || !albedo || !kind || !moments_xyzw || width == 0u || height == 0u || width > 65535u || height > 65535u) return RPT_EINVAL;
    rpt_denoise_var_params vp = DN_VAR_DEFAULTS;
    vp.clamp_scale = clamp_scale; vp.clamp_floor = clamp_floor; vp.clamp_radius = clamp_radius;
    std::string error;
    if (check_var_params(vp, 0u, error)) { rpt_create_error() = error; return RPT_EINVAL; }
    const size_t n = (size_t)width * height;
    std::vector<float4> g1(n), a(n), mo(n);
    for (size_t i = 0; i < n; ++i) {
        g1[i] = make_float4(0.0f, 0.0f, 0.0f, rptm::u2f(kind[i]));
        a[i] = make_float4(albedo[3 * i], albedo[3 * i + 1], albedo[3 * i + 2], 0.0f);
        mo[i] = make_float4(moments_xyzw[4 * i], moments_xyzw[4 * i + 1], moments_xyzw[4 * i + 2], moments_xyzw[4 * i + 3]);
    }
    const FfView fv{width, height, clamp_radius, demodulated != 0u ? 1u : 0u, clamp_scale, clamp_floor, mo.data(), nullptr, g1.data(), a.data()};
    for (size_t i = 0; i < n; ++i) {
        FfOut f{f3(mean_rgb[3 * i], mean_rgb[3 * i + 1], mean_rgb[3 * i + 2]), mo[i], false};
        if (clamp_scale != 0.0f) f = ff_pixel(fv, (uint32_t)(i % width), (uint32_t)(i / width), f.c, counts ? counts[i] : (float)samples, mo[i]);
        if (out_rgb) { out_rgb[3 * i] = f.c.x; out_rgb[3 * i + 1] = f.c.y; out_rgb[3 * i + 2] = f.c.z; }
        if (out_moments_xyzw) { out_moments_xyzw[4 * i] = f.m.x; out_moments_xyzw[4 * i + 1] = f.m.y; out_moments_xyzw[4 * i + 2] = f.m.z; out_moments_xyzw[4 * i + 3] = f.m.w; }
        if (out_mask) out_mask[i] = f.clamped ? 1u : 0u;
    }
    return RPT_OK;
}

}  // extern "C"
