/*
 * rpt_lens.hip — the thin-lens camera (include/rpt/rpt.h rpt_set_camera_lens; k_lens.h lens_ray): the setting, and the kernels a render call launches in place
 * of the reference camera's while the lens is active —
 *   k_generate_lens                           k_generate_first's full pass over the slots (k_sky_generate.h), every first path with the lens's ray
 *   k_lens_complete, k_lens_complete_moments  the text of the completion kernels (k_complete_body.h) with the restart of a finished slot through the lens
 *   k_dn_camera_rays_lens                     the centre rays of the denoiser's guides: pixel centre through the LENS CENTRE with the field of view
 *   k_lens_rays                               the test hook rpt_debug_lens_rays
 * A translation unit of its own, and the lens an argument of its own: no kernel of the other units, and no struct one of them takes by value, changes for it.
 * A path starts in few places: with two or more slots per pixel (plan_slots, rpt_hip.hip, sees to that) the side stages only park finished samples
 * (k_path.h finish_in_side_stage), so the opening pass and the completion kernels are all that has to know the lens; the lens sample comes from the two
 * entries of the LDS table no path reads, so a path goes on at dimension 2 (RPT_FRESH_FLAGS) and the shade, sky and shadow stages are the ones they were.
 */
#include <cmath>
#include <cstring>

#include "rpt_ctx.h"

#define RPT_COMPLETE_HELPERS_ONLY        /* (k_complete and k_complete_moments are plain kernels of rpt_hip.hip) */
#include "k_complete.h"
#include "k_lens.h"

static_assert(sizeof(rpt_camera_lens) == 16, "rpt_camera_lens: three floats and a reserved word");

/* k_path.h start_path / start_first_path with the lens's ray */
__device__ __forceinline__ void start_path_lens(const DevLens &lens, const DevState &st, const DevConfig &cfg, uint32_t slot, uint32_t n, uint32_t offset, uint32_t todo_after) {
    uint32_t pxy = st.pixel_xy[slot_pix(st, slot)];
    F3 ro, rd;
    lens_ray(cfg, lens, pxy & 0xffffu, pxy >> 16, n + offset, ro, rd);
    st.ray_a[slot] = make_float4(ro.x, ro.y, ro.z, rd.x);
    st.ray_b[slot] = make_float2(rd.y, rd.z);
    set_hit_word(st, slot, HIT_PENDING);
    st.thr[slot] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(MAKE_FLAGS(0u, 0u, 2u)));
    st.rad[slot] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(todo_after));
}
__device__ __forceinline__ void start_first_path_lens(const DevLens &lens, const DevState &st, const DevConfig &cfg, uint32_t slot, uint32_t n, uint32_t offset) {
    uint32_t pxy = st.pixel_xy[slot_pix(st, slot)];
    F3 ro, rd;
    lens_ray(cfg, lens, pxy & 0xffffu, pxy >> 16, n + offset, ro, rd);
    st.ray_a[slot] = make_float4(ro.x, ro.y, ro.z, rd.x);
    st.ray_b[slot] = make_float2(rd.y, rd.z);
    set_hit_word(st, slot, HIT_PENDING);
}

/* k_generate_first (k_sky_generate.h) as the pass over all slots — the call's counters, the undrained check, the padding slots, max_bounces == 0 — with
 * start_first_path_lens.  Launched with at least two slots per pixel only. */
__global__ __launch_bounds__(RPT_BLOCK) void k_generate_lens(DevState st, DevQueues q, DevConfig cfg, uint32_t n_samples, DevStats *stats, DevLens lens) {
    uint32_t slot = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (blockIdx.x == 0u)                                     /* queue counters and flags of the new call (no kernel of this call has run yet) */
        for (uint32_t k = threadIdx.x; k < (uint32_t)Q_COUNT; k += RPT_BLOCK) q.count[k] = 0u;
    if (blockIdx.x == 0u && threadIdx.x < RPT_Q_SHARDS) q.sky_cnt[threadIdx.x * RPT_Q_SHARD_STRIDE] = q.shadow_cnt[threadIdx.x * RPT_Q_SHARD_STRIDE] = 0u;
    if (slot >= st.n_slots) return;
    if (__float_as_uint(st.hit[slot].y) != HIT_IDLE) atomicAdd(&stats->undrained, 1ull);      /* (a sample the previous call left in flight: k_generate_first) */
    const uint32_t S = 1u << st.group_shift, k = slot_k(st, slot), pix = slot_pix(st, slot);
    if (pix >= st.n_pixels) {                                 /* padding of the last chunk of 64 pixels: never holds a path */
        set_hit_word(st, slot, HIT_IDLE);
        return;
    }
    uint2 rs = st.rng[pix];
    if (cfg.c.max_bounces == 0u) {
        /* the bounce loop never runs (lib.rs:62): every sample adds (0,0,0,1) */
        if (k == 0u) {
            float4 acc = st.accum[pix];
            for (uint32_t s = 0; s < n_samples; ++s) acc.w += 1.0f;
            st.accum[pix] = acc;
            rs.x += n_samples;
            st.rng[pix] = rs;
        }
        set_hit_word(st, slot, HIT_IDLE);
        return;
    }
    uint32_t count = n_samples > k ? (n_samples - k + S - 1u) / S : 0u;
    if (count == 0u) set_hit_word(st, slot, HIT_IDLE);
    else start_first_path_lens(lens, st, cfg, slot, rs.x + k, rs.y);      /* (owes count - 1 more: first_path_todo) */
}

/* the completion kernels: k_complete.h's two builds with the lens as one more argument and the lens's start of a path.  Named k_lens_complete*, not
 * k_complete_*: tests/test_kernel_resources.py and tests/test_kernel_resources_moments.py find the default completion kernels by the prefix "k_complete" and
 * hold that there are exactly two; tests/test_kernel_resources_camera_lens.py pins these. */
#define RPT_LENS(...) __VA_ARGS__
#define RPT_COMPLETE_START(...) start_path_lens(lens, __VA_ARGS__)
#define RPT_COMPLETE_KERNEL k_lens_complete
#define RPT_COMPLETE_DIRECT_ROWS complete_direct_rows_lens
#define RPT_COMPLETE_RESTART_ROWS complete_restart_rows_lens
#define RPT_MOM(...)
#include "k_complete_body.h"
#undef RPT_COMPLETE_KERNEL
#undef RPT_COMPLETE_DIRECT_ROWS
#undef RPT_COMPLETE_RESTART_ROWS
#undef RPT_MOM
#define RPT_COMPLETE_KERNEL k_lens_complete_moments
#define RPT_COMPLETE_DIRECT_ROWS complete_direct_rows_moments_lens
#define RPT_COMPLETE_RESTART_ROWS complete_restart_rows_moments_lens
#define RPT_MOM(...) __VA_ARGS__
#include "k_complete_body.h"
#undef RPT_COMPLETE_KERNEL
#undef RPT_COMPLETE_DIRECT_ROWS
#undef RPT_COMPLETE_RESTART_ROWS
#undef RPT_MOM
#undef RPT_COMPLETE_START
#undef RPT_LENS

/* k_dn_camera_rays (k_denoise.h) with lens_ray_centre */
__global__ __launch_bounds__(RPT_BLOCK) void k_dn_camera_rays_lens(DevConfig cfg, DevLens lens, const uint32_t *order, uint32_t n, float *origins, float *dirs) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t pxy = order[i];
    F3 ro, rd;
    lens_ray_centre(cfg, lens, pxy & 0xffffu, pxy >> 16, ro, rd);
    const size_t j = 3u * (size_t)i;
    origins[j] = ro.x; origins[j + 1u] = ro.y; origins[j + 2u] = ro.z;
    dirs[j] = rd.x; dirs[j + 1u] = rd.y; dirs[j + 2u] = rd.z;
}

/* rpt_debug_lens_rays: lens_ray for chosen (pixel, key) pairs */
__global__ __launch_bounds__(RPT_BLOCK) void k_lens_rays(DevConfig cfg, DevLens lens, const uint32_t *pixels_xy, const uint32_t *keys, uint32_t n, float *origins, float *dirs) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t pxy = pixels_xy[i];
    F3 ro, rd;
    lens_ray(cfg, lens, pxy & 0xffffu, pxy >> 16, keys[i], ro, rd);
    const size_t j = 3u * (size_t)i;
    origins[j] = ro.x; origins[j + 1u] = ro.y; origins[j + 2u] = ro.z;
    dirs[j] = rd.x; dirs[j + 1u] = rd.y; dirs[j + 2u] = rd.z;
}

static DevLens dev_lens(const rpt_camera_lens &l) { return DevLens{l.tan_half_fov, l.aperture_radius, l.focus_distance}; }
static const rpt_camera_lens LENS_DEFAULT = {1.0f, 0.0f, 1.0f, 0u};

/* what rpt_set_camera_lens refuses of the record itself, named after `who` */
static int check_lens(const rpt_camera_lens &l, std::string &error, const char *who) {
    const std::string w(who);
    if (!(std::isfinite(l.tan_half_fov) && l.tan_half_fov > 0.0f)) { error = w + ": tan_half_fov must be finite and above 0"; return RPT_EINVAL; }
    if (!(std::isfinite(l.aperture_radius) && l.aperture_radius >= 0.0f)) { error = w + ": aperture_radius must be finite and not negative"; return RPT_EINVAL; }
    if (l.aperture_radius > 0.0f && !(std::isfinite(l.focus_distance) && l.focus_distance > 0.0f)) { error = w + ": with an aperture, focus_distance must be finite and above 0"; return RPT_EINVAL; }
    if (l.reserved != 0u) { error = w + ": reserved must be 0"; return RPT_EINVAL; }
    return RPT_OK;
}

void rpt_launch_generate_lens(rpt_ctx *c, uint32_t n_samples, uint32_t blocks) {
    k_generate_lens<<<blocks, RPT_BLOCK, 0, c->stream>>>(c->state, c->queues, c->cfg, n_samples, c->dev_stats.p, dev_lens(c->lens));
}

void rpt_launch_complete_lens(rpt_ctx *c, uint32_t iteration, uint32_t final_pass, uint32_t waves, size_t lds_bytes) {
    if (c->moments_on) k_lens_complete_moments<<<waves, RPT_WAVE, lds_bytes, c->stream>>>(c->state, c->queues, c->cfg, iteration, final_pass, c->dev_stats.p, c->view ? c->view->moments : c->moments.p, dev_lens(c->lens));
    else k_lens_complete<<<waves, RPT_WAVE, lds_bytes, c->stream>>>(c->state, c->queues, c->cfg, iteration, final_pass, c->dev_stats.p, dev_lens(c->lens));
}

void rpt_launch_guide_rays_lens(rpt_ctx *c, const uint32_t *order, uint32_t n, float *origins, float *dirs) {
    k_dn_camera_rays_lens<<<rpt_blocks(n), RPT_BLOCK, 0, c->stream>>>(c->cfg, dev_lens(c->lens), order, n, origins, dirs);
}

extern "C" {

void rpt_camera_lens_default(rpt_camera_lens *out) {
    if (out) *out = LENS_DEFAULT;
}

int rpt_set_camera_lens(rpt_ctx *c, const rpt_camera_lens *lens) {
    if (!c) return RPT_EINVAL;
    const rpt_camera_lens l = lens ? *lens : LENS_DEFAULT;
    RPT_TRY(check_lens(l, c->error, "rpt_set_camera_lens"));
    if (c->has_config) RPT_TRY(rpt_lens_check_dimensions(c, c->cfg.c, l, "rpt_set_camera_lens"));
    if (c->async_pending) { c->error = "rpt_set_camera_lens: an asynchronous batch is pending (rpt_wait first)"; return RPT_EINVAL; }
    if (memcmp(&l, &c->lens, sizeof l) != 0) c->dn.guides_valid = false;      /* the denoiser's guides are the first hits of THIS camera: rebuilt at their next use */
    c->lens = l;
    return RPT_OK;
}

int rpt_camera_lens_get(rpt_ctx *c, rpt_camera_lens *out) {
    if (!c || !out) return RPT_EINVAL;
    *out = c->lens;
    return RPT_OK;
}

int rpt_debug_lens_rays_host(const rpt_tracing_config *config, const rpt_camera_lens *lens, const uint32_t *pixels_xy, const uint32_t *keys, size_t n, float *origins_out,
                             float *dirs_out) {
    std::string &error = rpt_create_error();
    if (!config || (n && (!pixels_xy || !keys || !origins_out || !dirs_out))) { error = "rpt_debug_lens_rays_host: null pointer"; return RPT_EINVAL; }
    if (config->width == 0u || config->height == 0u) { error = "rpt_debug_lens_rays_host: width and height must be above 0"; return RPT_EINVAL; }
    const rpt_camera_lens l = lens ? *lens : LENS_DEFAULT;
    RPT_TRY(check_lens(l, error, "rpt_debug_lens_rays_host"));
    DevConfig cfg{};
    cfg.c = *config;
    rpt_camera_matrix(config->cam_rotation, cfg.euler);
    const DevLens dl = dev_lens(l);
    for (size_t i = 0; i < n; ++i) {
        F3 ro, rd;
        lens_ray(cfg, dl, pixels_xy[i] & 0xffffu, pixels_xy[i] >> 16, keys[i], ro, rd);
        origins_out[3 * i] = ro.x; origins_out[3 * i + 1] = ro.y; origins_out[3 * i + 2] = ro.z;
        dirs_out[3 * i] = rd.x; dirs_out[3 * i + 1] = rd.y; dirs_out[3 * i + 2] = rd.z;
    }
    return RPT_OK;
}

int rpt_debug_lens_rays(rpt_ctx *c, const uint32_t *pixels_xy, const uint32_t *keys, size_t n, float *origins_out, float *dirs_out) {
    if (!c) return RPT_EINVAL;
    if (n && (!pixels_xy || !keys || !origins_out || !dirs_out)) { c->error = "rpt_debug_lens_rays: null pointer"; return RPT_EINVAL; }
    if (!c->has_config) { c->error = "rpt_debug_lens_rays: rpt_set_config must precede it"; return RPT_EINVAL; }
    if (n > ((size_t)1 << 28)) { c->error = "rpt_debug_lens_rays: more than 2^28 rays"; return RPT_EINVAL; }
    if (n == 0) return RPT_OK;
    RPT_TRY(rpt_wait(c));
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<uint32_t> d_xy, d_keys;
    DevBuf<float> d_o, d_d;
    HIP_TRY(c, d_xy.from_host(pixels_xy, n)); HIP_TRY(c, d_keys.from_host(keys, n));
    HIP_TRY(c, d_o.alloc(3 * n)); HIP_TRY(c, d_d.alloc(3 * n));
    k_lens_rays<<<rpt_blocks(n), RPT_BLOCK, 0, c->stream>>>(c->cfg, dev_lens(c->lens), d_xy.p, d_keys.p, (uint32_t)n, d_o.p, d_d.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(origins_out, d_o.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(dirs_out, d_d.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
    return RPT_OK;
}

}  // extern "C"
