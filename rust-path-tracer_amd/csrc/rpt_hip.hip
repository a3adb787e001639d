/*
 * rpt_hip.hip — librpt_hip.so: the context's life cycle, configuration and
 * state, wavefront scheduling and read-outs of the C ABI of include/rpt/rpt.h
 * (the drop-in replacement of the gpgpu-rs/wgpu calls in the reference's
 * trace_gpu, src/trace.rs:136-224).  Scene preparation: rpt_scene.hip; the
 * traversal stages: rpt_traverse.hip; test hooks with kernels: rpt_debug.hip.
 *
 * Wavefront iteration (all queues of slot ids, all state SoA, no host round
 * trip per sample):
 *     traverse_nearest -> shade -> [traverse_shadow] -> sky -> generate
 * The host only learns the size of the next extension queue through a lagged
 * asynchronous read-back (pinned ring + events), so the GPU never idles on it.
 */
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "rpt_ctx.h"

#include "k_shade.h"             /* (the walk kernels of k_traverse.h are compiled in rpt_traverse.hip) */
#include "k_complete.h"
#include "k_sky_generate.h"
#include "k_image_order.h"

/* (read afresh by every rpt_create / scene-preparation call: a test process changes its environment between contexts) */
rpt_knobs rpt_read_knobs() {
    rpt_knobs k;
    auto num = [](const char *name, int lo, int hi, int otherwise) { const char *e = getenv(name); if (!e || !e[0]) return otherwise; const int v = atoi(e); return v < lo ? lo : (v > hi ? hi : v); };
    auto word = [](const char *name) { const char *e = getenv(name); return std::string(e ? e : ""); };
    k.stage_timing = num("RPT_STAGE_TIMING", 0, 2, 0);
    k.upload_timing = num("RPT_UPLOAD_TIMING", 0, 1, 0) == 1;
    k.slot_q_shift = num("RPT_SLOT_Q_SHIFT", 0, 5, -1);
    const std::string so = word("RPT_SHADOW_ORDER"), lo = word("RPT_LAST_ORDER");
    k.shadow_order = so == "near" ? 0 : (so == "fixed" ? 1 : -1);
    k.last_order = lo == "off" ? 4 : (lo == "near" ? 0 : (lo == "opaque" ? 1 : (lo == "small" ? 2 : (lo == "ratio" ? 3 : -1))));
    k.shade_compact = num("RPT_SHADE_COMPACT", 0, 1, -1);
    k.sky_strided = num("RPT_SKY_STRIDED", 0, 1 << 20, -1);
    k.stack_bits = num("RPT_STACK_BITS", 16, 32, 16);
    k.coop_leaves = num("RPT_COOP_LEAVES", 0, 1, -1);
    k.no_lds_scene = num("RPT_NO_LDS_SCENE", 0, 1, 0) == 1;
    k.bvh_team_min = num("RPT_BVH_TEAM_MIN", 2, 1 << 30, 0);
    return k;
}

thread_local std::string g_create_error;
std::string &rpt_create_error() { return g_create_error; }

/* rank-local slot order: tiles in ascending id (tile t -> rank t mod world),
 * inside a tile 8x8 pixel blocks row-major, inside a block row-major; pixels
 * outside the image are skipped.  One wave = one 8x8 block on full tiles, so
 * primary rays of a wave are coherent. */
void rpt_build_pixel_order(uint32_t W, uint32_t H, uint32_t rank, uint32_t world, std::vector<uint32_t> &out) {
    const uint32_t T = RPT_TILE, B = 8;
    uint32_t tiles_x = (W + T - 1) / T, tiles_y = (H + T - 1) / T;
    /* (count first, then plain stores: four million push_backs were 10 ms of rpt_set_config at 2048^2) */
    size_t total = 0;
    for (uint32_t t = rank; t < tiles_x * tiles_y; t += world) {
        const uint32_t tx = (t % tiles_x) * T, ty = (t / tiles_x) * T;
        total += (size_t)std::min(T, W - tx) * std::min(T, H - ty);
    }
    out.resize(total);
    uint32_t *at = out.data();
    for (uint32_t t = rank; t < tiles_x * tiles_y; t += world) {
        uint32_t tx = (t % tiles_x) * T, ty = (t / tiles_x) * T;
        for (uint32_t by = 0; by < T && ty + by < H; by += B)
            for (uint32_t bx = 0; bx < T && tx + bx < W; bx += B) {
                const uint32_t xs = std::min(B, W - (tx + bx)), ys = std::min(B, H - (ty + by));
                for (uint32_t y = 0; y < ys; ++y)
                    for (uint32_t x = 0; x < xs; ++x) *at++ = (tx + bx + x) | ((ty + by + y) << 16);
            }
    }
}

/* the tiles of that order, as the window rule of adaptive sampling takes them (k_adaptive.h AdTile): the same walk over the rank's tiles, so the two stay in step */
void rpt_build_tile_table(uint32_t W, uint32_t H, uint32_t rank, uint32_t world, std::vector<uint32_t> &out) {
    const uint32_t T = RPT_TILE, tiles_x = (W + T - 1) / T, tiles_y = (H + T - 1) / T;
    out.clear();
    uint32_t first = 0;
    for (uint32_t t = rank; t < tiles_x * tiles_y; t += world) {
        const uint32_t tx = (t % tiles_x) * T, ty = (t / tiles_x) * T, count = std::min(T, W - tx) * std::min(T, H - ty);
        out.insert(out.end(), {first, count, tx | (ty << 16), 0u});
        first += count;
    }
}

namespace {

constexpr int LAG = RPT_RING_LAG, RING = RPT_RING;

void rotation_y(float angle, float *m) {   /* Mat3::from_rotation_y, column-major */
    float s, c;
    rptm::sincosr(angle, s, c);
    m[0] = c; m[1] = 0.0f; m[2] = -s;
    m[3] = 0.0f; m[4] = 1.0f; m[5] = 0.0f;
    m[6] = s; m[7] = 0.0f; m[8] = c;
}
void rotation_x(float angle, float *m) {
    float s, c;
    rptm::sincosr(angle, s, c);
    m[0] = 1.0f; m[1] = 0.0f; m[2] = 0.0f;
    m[3] = 0.0f; m[4] = c; m[5] = s;
    m[6] = 0.0f; m[7] = -s; m[8] = c;
}
void mat3_mul_host(const float *a, const float *b, float *out) {   /* Mat3 * Mat3 = cols a*b.col */
    for (int c = 0; c < 3; ++c) {
        float v[3] = {b[3 * c], b[3 * c + 1], b[3 * c + 2]};
        for (int r = 0; r < 3; ++r) {
            float acc = a[r] * v[0];
            acc = acc + a[3 + r] * v[1];
            acc = acc + a[6 + r] * v[2];
            out[3 * c + r] = acc;
        }
    }
}

void release_state(rpt_ctx *c) {
    c->ray_a.release(); c->ray_b.release(); c->hit.release(); c->thr.release(); c->rad.release();
    c->mis_a.release(); c->mis_b.release();
    c->accum.release(); c->rng.release(); c->moments.release();
    c->q_sky.release(); c->q_count.release(); c->ray_shards.release();
    c->sh_o.release(); c->sh_d.release(); c->sh_c.release();
    c->pixel_xy.release();
    c->ad.release();
    c->image.release(); c->host_image.release(); c->untile_map.release();
    c->untile_key = 0;
    c->has_state = false;
    c->has_seeds = false;
}

/* Stream discipline: the context's stream is NON-BLOCKING, so nothing on the legacy default stream is ordered against it.
 * hipMemset of device memory may return before it has run; issued on the default stream it raced the first kernels of the
 * next render whenever other threads kept that stream busy with their own contexts (lost ray counts in
 * test_contexts_on_different_threads).  Hence: every fill is hipMemsetAsync ON THE CONTEXT'S STREAM; host-to-device copies
 * stay synchronous hipMemcpy (complete when they return) and are only issued after the stream has been drained. */
/* What rpt_set_config allocates: the per-PIXEL state (accumulators, rng, pixel coordinates) and the counters.  The per-SLOT path state is
 * allocated by the first rpt_render that needs it, at the size it needs (ensure_slot_state): a start-up — the reference's
 * trace_gpu(scene, 0 samples), benches/benchmark.rs:11-13 — allocates and touches no path state at all, a configuration without NEE no
 * shadow queue (48 bytes per slot) and no MIS carry (32), and the ceiling of samples in flight can be 256 per pixel without a context
 * that renders 32-sample batches paying for it (rounds 1-5 allocated up to 160 M slots x 180 bytes = 29 GB in rpt_set_config). */
int alloc_pixel_state(rpt_ctx *c) {
    const size_t np = c->n_pixels;
    HIP_TRY(c, c->accum.alloc(np)); HIP_TRY(c, c->rng.alloc(np));
    HIP_TRY(c, c->ray_shards.alloc(RPT_STAT_SHARDS * RPT_STAT_STRIDE));
    HIP_TRY(c, hipMemsetAsync(c->ray_shards.p, 0, RPT_STAT_SHARDS * RPT_STAT_STRIDE * sizeof(unsigned long long), c->stream));
    HIP_TRY(c, c->q_count.alloc(Q_WORDS));
    HIP_TRY(c, c->pixel_xy.alloc(np));
    if (np) HIP_TRY(c, hipMemcpy(c->pixel_xy.p, c->pixel_xy_host.data(), np * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemsetAsync(c->q_count.p, 0, Q_WORDS * sizeof(uint32_t), c->stream));
    DevState &s = c->state;
    s = DevState{};
    s.rng = c->rng.p; s.accum = c->accum.p; s.pixel_xy = c->pixel_xy.p; s.n_slots = c->n_slots;
    s.n_pixels = (uint32_t)np; s.group_shift = c->group_shift; s.q_shift = 0;
    DevQueues &q = c->queues;
    q = DevQueues{};
    q.ray_shards = c->ray_shards.p; q.count = c->q_count.p;
    q.sky_cnt = c->q_count.p + Q_COUNT; q.shadow_cnt = q.sky_cnt + RPT_Q_SHARDS * RPT_Q_SHARD_STRIDE;
    q.host_ring = c->host_ring_dev; q.ring_mask = RING - 1;
    /* up to this many queued misses the sky march runs 16 lanes per miss (re-clamped per call to that call's slot count) */
    q.sky_wide_limit = (uint32_t)std::min<size_t>(c->n_slots / 16, c->sky_wide_cfg);
    /* 1 = shade misses in the iteration that found them.  (Letting them pile up removed most of the near-empty sky launches on closed scenes, but the
     * parked pixels finish later and lengthen the tail: DarkCornell 3650 Mrays/s deferred vs 3928 eager in round 1; the knob went in round 6.) */
    q.sky_threshold = 1u; q.sky_at_end = 0u; q.known_length = 0u; q.implicit_zero = 0u;
    c->has_state = true;
    return RPT_OK;
}

static uint32_t padded_pixels(uint32_t n_pixels) { return (n_pixels + 63u) & ~63u; }      /* whole chunks of 64 pixels (k_common.h, slot_pix) */

/* one wave per chunk of 64 pixels (k_complete.h) */
static void launch_complete(rpt_ctx *c, uint32_t iteration, uint32_t final_pass) {
    if (rpt_lens_active(c)) {        /* (rpt_set_camera_lens: the same completions, a restarted path takes the lens's ray — rpt_lens.hip) */
        rpt_launch_complete_lens(c, iteration, final_pass, padded_pixels(c->n_pixels) / RPT_WAVE, complete_lds_bytes(1u << c->group_shift, c->state.q_shift));
        return;
    }
    if (c->moments_on) {             /* (rpt_set_moments: the same completion, the samples added to the moments record too — the view's compact one in a masked pass) */
        k_complete_moments<<<padded_pixels(c->n_pixels) / RPT_WAVE, RPT_WAVE, complete_lds_bytes(1u << c->group_shift, c->state.q_shift), c->stream>>>(c->state, c->queues, c->cfg, iteration,
                                                                                                                                 final_pass, c->dev_stats.p, c->view ? c->view->moments : c->moments.p);
        return;
    }
    k_complete<<<padded_pixels(c->n_pixels) / RPT_WAVE, RPT_WAVE, complete_lds_bytes(1u << c->group_shift, c->state.q_shift), c->stream>>>(c->state, c->queues, c->cfg, iteration, final_pass,
                                                                                                                     c->dev_stats.p);
}

/* returns the shade launches it made: 1, or 0 where the walk ended its paths itself (rpt_launch_nearest) */
template <int NEE, bool TEXTURED>
uint32_t launch_iteration(rpt_ctx *c, uint32_t iteration, uint32_t blocks, bool complete_each, bool sky_now) {
    hipStream_t s = c->stream;
    StageTimer &t = c->timing;
    t.mark(s, StageTimer::NONE, StageTimer::AT_2);
    /* the consumers of a side queue cover its POSITIONS: up to RPT_Q_SLACK more than there are slots (k_common.h) */
    const uint32_t blocks_q = rpt_blocks(c->n_slots + RPT_Q_SLACK);
    /* (the shade stage's last_iteration, k_shade.h: in a batch of known length iteration k is bounce k of every path) */
    const bool ended = rpt_launch_nearest(c, iteration, NEE == RPT_NEE_NONE && c->queues.known_length != 0u && iteration != 0u && iteration + 1u >= c->cfg.c.max_bounces,
                                          iteration == 0u && !rpt_lens_scatters_origins(c) /* (an aperture: the camera rays leave a disk, the plain walk takes them) */,
                                          iteration == 0u && c->first_walk_starts);
    t.mark(s, RPT_STAGE_TRAVERSE, StageTimer::AT_1 | StageTimer::AT_2);
    if (!ended) {                                           /* (ended: nothing is left for a shade stage, every path of the launch is HIT_DONE or waits in the sky queue) */
        c->last_shade_variant = (c->volumes_in_use || c->force_volume_kernels) ? 2u : ((c->models_in_use || c->force_model_kernels) ? 1u : 0u);
        if (NEE != RPT_NEE_NONE && (!c->punctual_lights_host.empty() || c->force_punctual_kernels)) c->last_shade_variant = 3u;
        if (c->last_shade_variant == 3u) rpt_launch_shade_punctual(c, iteration, blocks);                  /* (rpt_set_punctual_lights: NEE has punctual lights to pick) */
        else if (c->last_shade_variant == 2u) rpt_launch_shade_volumes(c, iteration, blocks);                   /* (rpt_set_material_volumes: some Glass material absorbs) */
        else if (c->last_shade_variant == 1u) rpt_launch_shade_models(c, iteration, blocks);               /* (rpt_set_material_models: some material is not PBR) */
        else if (c->shade_compact) k_shade<NEE, TEXTURED, true><<<(c->n_slots + RPT_BLOCK * RPT_SHADE_ROUNDS - 1) / (RPT_BLOCK * RPT_SHADE_ROUNDS), RPT_BLOCK, 0, s>>>(c->scene, c->state, c->queues, c->cfg, iteration, c->dev_stats.p, c->call_samples);
        else k_shade<NEE, TEXTURED, false><<<blocks, RPT_BLOCK, 0, s>>>(c->scene, c->state, c->queues, c->cfg, iteration, c->dev_stats.p, c->call_samples);
    }
    /* generations are completed (and the next samples started) after every shade stage only where slots take more than one
     * sample in this call; a batch of known length completes them once, after its last iteration (render_impl) */
    if (complete_each) launch_complete(c, iteration, 0u);
    t.mark(s, RPT_STAGE_SHADE, StageTimer::AT_1);
    if (NEE != RPT_NEE_NONE) rpt_launch_shadow(c);          /* the any-hit walk of the queued shadow rays (+ k_shadow_resolve behind the streamed LDS walk) */
    t.mark(s, RPT_STAGE_SHADOW, StageTimer::AT_1);
    if (c->queues.sky_at_end == 0u || sky_now) {
        if (c->sky_strided && blocks > c->sky_blocks) k_sky<true><<<c->sky_blocks, RPT_BLOCK, 0, s>>>(c->scene, c->state, c->queues, c->cfg, iteration, c->dev_stats.p);
        else k_sky<false><<<blocks_q, RPT_BLOCK, 0, s>>>(c->scene, c->state, c->queues, c->cfg, iteration, c->dev_stats.p);
    }
    t.mark(s, RPT_STAGE_SKY, StageTimer::AT_1);
    return ended ? 0u : 1u;
}

/* one iteration with the shade stage built for the context's NEE mode and scene (the walks pick their stack width themselves: rpt_traverse.hip) */
static uint32_t dispatch_iteration(rpt_ctx *c, uint32_t iteration, uint32_t blocks, bool complete_each, bool sky_now) {
    const bool tex = c->scene.textured != 0u;
    switch (c->cfg.nee_mode) {
        case RPT_NEE_MIS:
            return tex ? launch_iteration<RPT_NEE_MIS, true>(c, iteration, blocks, complete_each, sky_now)
                       : launch_iteration<RPT_NEE_MIS, false>(c, iteration, blocks, complete_each, sky_now);
        case RPT_NEE_DIRECT:
            return tex ? launch_iteration<RPT_NEE_DIRECT, true>(c, iteration, blocks, complete_each, sky_now)
                       : launch_iteration<RPT_NEE_DIRECT, false>(c, iteration, blocks, complete_each, sky_now);
        default:
            return tex ? launch_iteration<RPT_NEE_NONE, true>(c, iteration, blocks, complete_each, sky_now)
                       : launch_iteration<RPT_NEE_NONE, false>(c, iteration, blocks, complete_each, sky_now);
    }
}

}  // namespace

/* DevConfig::euler of a configuration's cam_rotation (x = pitch, y = yaw): column-major RotY(yaw) * RotX(pitch) */
void rpt_camera_matrix(const float *cam_rotation, float *euler_out) {
    float ry[9], rx[9];
    rotation_y(cam_rotation[1], ry);
    rotation_x(cam_rotation[0], rx);
    mat3_mul_host(ry, rx, euler_out);
}

uint64_t rpt_config_dimensions(const rpt_tracing_config &cfg) {
    const uint32_t nee_mode = cfg.nee <= 2u ? cfg.nee : 0u;
    const uint64_t per_bounce = 3u + (nee_mode ? 4u : 0u);
    const uint64_t rr = cfg.max_bounces > cfg.min_bounces + 1u ? cfg.max_bounces - 1u - cfg.min_bounces : 0u;
    return 2u + (uint64_t)cfg.max_bounces * per_bounce + rr;
}

int rpt_lens_check_dimensions(rpt_ctx *c, const rpt_tracing_config &cfg, const rpt_camera_lens &lens, const char *who) {
    if (!(lens.aperture_radius > 0.0f) || rpt_config_dimensions(cfg) < 31u) return RPT_OK;
    c->error = std::string(who) + ": the configuration needs all 31 LDS dimensions and the lens has an aperture: its sample takes entry 31 of the reference's table "
               "(aperture_radius = 0, or a configuration of at most 30 dimensions)";
    return RPT_ECONFIG;
}

/* The per-slot arrays, for a render call over `n` slots: grown (never shrunk) to what the call needs — the path state always, the shadow
 * queue when the configuration has NEE, the MIS carry when it is MIS.  Growing waits for whatever is in flight, frees the old arrays first
 * and leaves every slot idle; between render calls every slot IS idle, so nothing is carried over. */
int ensure_slot_state(rpt_ctx *c, size_t n, bool need_shadow, bool need_mis) {
    const bool grow = c->hit.n < n, grow_shadow = need_shadow && c->sh_o.n < n + RPT_Q_SLACK, grow_mis = need_mis && c->mis_a.n < n;
    if (grow || grow_shadow || grow_mis) {
        SectionTimer sections("path state");
        if (c->async_pending) RPT_TRY(rpt_wait(c));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        sections.mark("drain");
        if (grow) {
            c->ray_a.release(); c->ray_b.release(); c->hit.release(); c->thr.release(); c->rad.release(); c->q_sky.release();
            HIP_TRY(c, c->ray_a.alloc(n)); HIP_TRY(c, c->ray_b.alloc(n)); HIP_TRY(c, c->hit.alloc(n));
            HIP_TRY(c, c->thr.alloc(n)); HIP_TRY(c, c->rad.alloc(n));
            HIP_TRY(c, c->q_sky.alloc(n + RPT_Q_SLACK));     /* side queues: positions, not entries (k_common.h: sharded queues) */
            sections.mark("alloc_path_state");
            k_fill_idle<<<rpt_blocks(n), RPT_BLOCK, 0, c->stream>>>(c->hit.p, (uint32_t)n);   /* nothing in flight */
            HIP_TRY(c, hipGetLastError());
        }
        if (grow_shadow) {
            c->sh_o.release(); c->sh_d.release(); c->sh_c.release();
            HIP_TRY(c, c->sh_o.alloc(n + RPT_Q_SLACK)); HIP_TRY(c, c->sh_d.alloc(n + RPT_Q_SLACK)); HIP_TRY(c, c->sh_c.alloc(n + RPT_Q_SLACK));
        }
        if (grow_mis) {
            c->mis_a.release(); c->mis_b.release();
            HIP_TRY(c, c->mis_a.alloc(n)); HIP_TRY(c, c->mis_b.alloc(n));
        }
        sections.mark("alloc_queues_carries");
    }
    DevState &s = c->state;
    s.ray_a = c->ray_a.p; s.ray_b = c->ray_b.p; s.hit = c->hit.p; s.thr = c->thr.p; s.rad = c->rad.p;
    s.mis_a = c->mis_a.p; s.mis_b = c->mis_b.p;
    DevQueues &q = c->queues;
    q.sky = c->q_sky.p; q.sh_o = c->sh_o.p; q.sh_d = c->sh_d.p; q.sh_c = c->sh_c.p;
    return RPT_OK;
}

/* "nothing in flight": the queue counters zeroed and every slot of the current call idle, on the context's stream */
int rpt_idle_all_slots(rpt_ctx *c) {
    hipStream_t s = c->stream;
    HIP_TRY(c, hipMemsetAsync(c->q_count.p, 0, Q_WORDS * sizeof(uint32_t), s));
    k_fill_idle<<<rpt_blocks(c->n_slots), RPT_BLOCK, 0, s>>>(c->hit.p, c->n_slots);
    return RPT_OK;
}

/* rpt_reset: the caller's row-major seeds (and accumulators, when a render resumes) into the rank's tile-major pixel order */
__global__ __launch_bounds__(RPT_BLOCK) void k_reset_gather(const uint32_t *pixel_xy, uint32_t n_pixels, uint32_t width, const uint2 *seed, const float4 *accum_init /* nullable */,
                                                            uint2 *rng, float4 *accum) {
    const uint32_t s = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (s >= n_pixels) return;
    const size_t i = rpt_pixel_index(pixel_xy[s], width);
    rng[s] = seed[i];
    accum[s] = accum_init ? accum_init[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

extern "C" {

int rpt_abi_version(void) { return RPT_ABI_VERSION; }

#ifndef RPT_BUILD_FINGERPRINT
#define RPT_BUILD_FINGERPRINT "unknown"
#endif
const char *rpt_build_fingerprint(void) { return RPT_BUILD_FINGERPRINT; }

int rpt_device_info(int device_id, uint32_t *compute_units_out, uint32_t *clock_khz_out) {
    int cus = 0, khz = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess ||
        hipDeviceGetAttribute(&khz, hipDeviceAttributeClockRate, device_id) != hipSuccess) {
        g_create_error = "rpt_device_info: no such HIP device";
        return RPT_ENODEV;
    }
    if (compute_units_out) *compute_units_out = (uint32_t)cus;
    if (clock_khz_out) *clock_khz_out = (uint32_t)khz;
    return RPT_OK;
}

const char *rpt_last_error(rpt_ctx *ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int rpt_create(int device_id, rpt_ctx **out) {
    if (!out) { g_create_error = "null out pointer"; return RPT_EINVAL; }
    *out = nullptr;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev == 0) {
        g_create_error = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return RPT_ENODEV;
    }
    if (device_id < 0 || device_id >= n_dev) { g_create_error = "device id out of range"; return RPT_EINVAL; }
    e = hipSetDevice(device_id);
    if (e != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return RPT_EHIP; }
    auto *c = new rpt_ctx();
    c->device = device_id;
    /* (a context that cannot be completed goes the way every context goes: rpt_destroy copes with whatever is missing) */
    auto fail = [c](int code, const std::string &why) { g_create_error = why; rpt_destroy(c); return code; };
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(RPT_EHIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    if ((e = c->host_ring.alloc(RING, hipHostMallocMapped)) != hipSuccess ||
        (e = hipHostGetDevicePointer(reinterpret_cast<void **>(&c->host_ring_dev), c->host_ring.p, 0)) != hipSuccess)
        return fail(RPT_EHIP, std::string("hipHostMalloc(mapped): ") + hipGetErrorString(e));
    memset(c->host_ring.p, 0, RING * sizeof(unsigned long long));
    if (c->dev_stats.alloc(1) != hipSuccess || hipMemsetAsync(c->dev_stats.p, 0, sizeof(DevStats), c->stream) != hipSuccess)
        return fail(RPT_ENOMEM, "device allocation failed");
    c->knobs = rpt_read_knobs();
    c->timing.level = c->knobs.stage_timing;          /* (0, StageTimer::AT_1, StageTimer::AT_2) */
    if (c->knobs.shade_compact >= 0) { c->shade_compact_mode = c->knobs.shade_compact; c->shade_compact = c->shade_compact_mode == 1; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) c->stream_max_blocks = 2u * (uint32_t)prop.multiProcessorCount;
    c->sky_blocks = 16u * c->stream_max_blocks / 2u;       /* 16 workgroups of 256 per CU: the sky stage strides over its queue */
    if (c->knobs.sky_strided >= 0) {
        c->sky_strided_mode = c->knobs.sky_strided != 0 ? 1 : 0;
        c->sky_strided = c->sky_strided_mode == 1;
        if (c->knobs.sky_strided > 1) c->sky_blocks = (uint32_t)c->knobs.sky_strided;
    }
    *out = c;
    return RPT_OK;
}

void rpt_destroy(rpt_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    rpt_comm_release(c);                 /* (destroys the RCCL communicator: before anything else goes) */
    rpt_denoise_release(c, true);
    c->timing.clear();                   /* (its events go while the device is current and the stream they were recorded on exists) */
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                            /* (frees every buffer of the context) */
}

/* the configuration the context has, if it has one, set again: everything derived from it is derived afresh */
static int reapply_config(rpt_ctx *c) {
    if (!c->has_config) return RPT_OK;
    const rpt_tracing_config cfg = c->cfg.c;
    c->has_config = false;
    return rpt_set_config(c, &cfg);
}

int rpt_set_partition(rpt_ctx *c, uint32_t rank, uint32_t world_size) {
    if (!c) return RPT_EINVAL;
    if (world_size == 0 || rank >= world_size) { c->error = "rank must be < world_size"; return RPT_EINVAL; }
    if (c->rank == rank && c->world == world_size) return RPT_OK;      /* nothing changes: keep the state */
    c->rank = rank;
    c->world = world_size;
    return reapply_config(c);            /* re-derive the slot order for the new partition */
}

int rpt_set_config(rpt_ctx *c, const rpt_tracing_config *cfg) {
    if (!c || !cfg) return RPT_EINVAL;
    if (cfg->width == 0 || cfg->height == 0 || cfg->width > 65535u || cfg->height > 65535u) {
        c->error = "width/height must be in 1..65535";
        return RPT_EINVAL;
    }
    uint32_t nee_mode = cfg->nee <= 2u ? cfg->nee : 0u;
    if (cfg->max_bounces > 255u) { c->error = "max_bounces > 255"; return RPT_ECONFIG; }
    {
        /* LDS dimension budget (kernels/src/rng.rs:20-21,51-54): the CPU reference panics past 31 */
        const uint64_t dims = rpt_config_dimensions(*cfg);
        if (dims > 31u) {
            c->error = "config needs " + std::to_string(dims) + " LDS dimensions; the reference's table has 31 usable";
            return RPT_ECONFIG;
        }
        RPT_TRY(rpt_lens_check_dimensions(c, *cfg, c->lens, "rpt_set_config"));
    }
    HIP_TRY(c, hipSetDevice(c->device));
    bool resized = !c->has_config || c->cfg.c.width != cfg->width || c->cfg.c.height != cfg->height;
    c->cfg.c = *cfg;
    c->cfg.nee_mode = nee_mode;
    rpt_camera_matrix(cfg->cam_rotation, c->cfg.euler);
    rotation_y(rptm::atan2r(cfg->sun_direction[2], cfg->sun_direction[0]), c->cfg.sky_rot);
    c->dn.guides_valid = false;          /* the denoiser's guides are the first hits of THIS camera: rebuilt at their next use */
    if (resized || !c->has_state) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        release_state(c);
        if (resized) rpt_denoise_release(c, false);
        rpt_build_pixel_order(cfg->width, cfg->height, c->rank, c->world, c->pixel_xy_host);
        c->n_pixels = (uint32_t)c->pixel_xy_host.size();
        /* Samples of one pixel in flight.  The GPU holds 8 192 waves = 0.5 M paths at once and ray costs inside a
         * launch vary widely, so a launch of only 1-2 x that ends in a long half-empty tail (measured 4.3 of 8 waves
         * per SIMD resident on average with 1 M slots); up to 16 M slots (~3 GB of path state at 200 B/slot, nothing
         * on a 288 GB part) make the tail a small fraction and quarter the number of launches per batch:
         * DarkCornell 1024^2 4.84 -> 6.33 Grays/s for S = 1 -> 16.  The image does not depend on S. */
        /* This is the MOST a call may use (the arrays are sized for it); each rpt_render call keeps
         * min(this, next power of two >= its n_samples) slots per pixel busy — slots without a sample would only be
         * scanned (16 spp on 32 slots per pixel: 6.0 instead of 8.2 Grays/s).  Up to 32 slots per pixel and 32 M
         * slots: with the reference's default batch of 32 samples (sync_rate, src/trace.rs:75) a rank that owns 1/8
         * of a 1024^2 image then has 4 M paths in flight (7.2 instead of 6.6 Grays/s per GPU). */
        /* Up to 256 since round 6 (k_complete.h counts the finished slots of a pixel instead of keeping a 32-bit mask): a rank that owns 1/8
         * of a 1024^2 image runs a 256-sample batch as the same 33 M-slot launches as the whole image runs 32 — the fixed costs of a batch
         * (11 launches, drain tails) no longer weigh 8 x as much.  The arrays are allocated by the render call that needs them, at its size. */
        uint32_t S = 1;
        if (c->samples_in_flight_request > 0) {
            while (S < (uint32_t)c->samples_in_flight_request && S < RPT_MAX_SAMPLES_IN_FLIGHT) S <<= 1;
        } else {
            /* as many as fit in RPT_MAX_SLOTS (160 M slots x 70 - 150 B of path state and queues).  Round 1
             * stopped at 32 M and used S = 1 from 3 M pixels up, where more slots only cost: with one ray per lane the dead
             * slots of an open scene were walked as empty lanes.  The streamed walks skip them, and measured now (32-spp
             * batches): PBRTest 2048^2 4090 / 4354 / 4505 / 4537 / 4709 Mrays/s for S = 1 / 4 / 8 / 16 / 32, VeachMIS 1080p
             * 4388 / 4757 / 4892 for S = 8 / 16 / 32, the 1 M-triangle stand-in at 2048^2 994 / 1578 for S = 1 / 16. */
            while (S < RPT_MAX_SAMPLES_IN_FLIGHT && (uint64_t)c->n_pixels * S * 2u <= c->max_slots_budget) S <<= 1;
        }
        c->max_group_shift = 0;
        while ((1u << c->max_group_shift) < S) c->max_group_shift += 1;
        c->max_slots = padded_pixels(c->n_pixels) << c->max_group_shift;       /* chunks of 64 pixels x S slots (k_common.h, slot_pix) */
        c->group_shift = std::min(c->max_group_shift, 5u);                     /* (until the first render call says how many it needs) */
        c->n_slots = padded_pixels(c->n_pixels) << c->group_shift;
        RPT_TRY(alloc_pixel_state(c));
        /* fresh accumulators; seeds must come from rpt_reset */
        if (c->n_pixels) {
            HIP_TRY(c, hipMemsetAsync(c->accum.p, 0, c->n_pixels * sizeof(float4), c->stream));
            HIP_TRY(c, hipMemsetAsync(c->rng.p, 0, c->n_pixels * sizeof(uint2), c->stream));
        }
        c->samples = 0;
        c->counts_nonuniform = false;
        c->accum_epoch += 1;
        RPT_TRY(rpt_moments_reset(c));       /* (moments on: a record for the new pixel count, zeroed like the accumulator) */
    }
    c->has_config = true;
    return RPT_OK;
}

int rpt_reset(rpt_ctx *c, const rpt_rng_state *seed, const float *accum_init, uint32_t samples_init) {
    if (!c) return RPT_EINVAL;
    if (!c->has_config || !c->has_state) { c->error = "rpt_set_config must precede rpt_reset"; return RPT_EINVAL; }
    if (!seed) { c->error = "null seed buffer"; return RPT_EINVAL; }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    /* The caller's row-major buffers go up as they are; a kernel gathers them into this rank's tile-major pixel order (rounds 1-5 gathered on the host:
     * two loops over every pixel and 24 bytes per pixel of staging, 20 ms of a 2048^2 reset).  No accum_init: the accumulators are simply zeroed. */
    const uint32_t W = c->cfg.c.width, H = c->cfg.c.height;
    const size_t n = c->n_pixels, whole = (size_t)W * H;
    if (n) {
        DevBuf<uint2> d_seed;
        DevBuf<float4> d_acc;
        HIP_TRY(c, d_seed.from_host(seed, whole));
        if (accum_init) HIP_TRY(c, d_acc.from_host(accum_init, whole));
        k_reset_gather<<<rpt_blocks(n), RPT_BLOCK, 0, c->stream>>>(c->pixel_xy.p, (uint32_t)n, W, d_seed.p, d_acc.p, c->rng.p, c->accum.p);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(c->stream));             /* (before the staging buffers are freed) */
    }
    HIP_TRY(c, hipMemsetAsync(c->dev_stats.p, 0, sizeof(DevStats), c->stream));
    HIP_TRY(c, hipMemsetAsync(c->ray_shards.p, 0, RPT_STAT_SHARDS * RPT_STAT_STRIDE * sizeof(unsigned long long), c->stream));
    RPT_TRY(rpt_moments_reset(c));           /* (not resumed: with accum_init the record counts the samples rendered from here on) */
    c->samples = accum_init ? samples_init : 0u;
    c->counts_nonuniform = false;
    c->accum_epoch += 1;
    c->has_seeds = true;
    c->stats = rpt_stats{};
    return RPT_OK;
}

/* Read the device counters after a synchronisation: reports samples a fixed-length batch left in flight, and picks the
 * shade-stage variant for the batches to come.  Packing the traversed slots per workgroup before shading (k_shade<..,
 * COMPACT>) pays when most slots of a pass are parked — measured: PBRTest 2048^2 (0.94 sky hits per sample) shade 86.6 ->
 * 68.5 ms per 4 batches — and costs on scenes whose paths stay alive (DarkCornell 31.4 -> 39.2; VeachMIS with 0.84: even):
 * so it is switched on when more than RPT_SHADE_COMPACT_AT (default 0.7) of the samples rendered since the last reset
 * ended in the sky.  Either variant produces the same image bit for bit. */
static int refresh_device_stats(rpt_ctx *c, const char *what) {
    DevStats ds;
    HIP_TRY(c, hipMemcpy(&ds, c->dev_stats.p, sizeof(ds), hipMemcpyDeviceToHost));
    if (ds.undrained != 0ull) {
        c->error = std::string(what) + ": " + std::to_string(ds.undrained) + " samples were still in flight after its iterations (internal error)";
        return RPT_EHIP;
    }
    if (c->shade_compact_mode < 0 && c->stats.samples != 0ull)
        c->shade_compact = (double)ds.sky_evals > c->shade_compact_at * (double)c->stats.samples;
    /* the sky stage walks its queue with a small fixed grid when misses are rare (k_sky<STRIDED>: see there) */
    if (c->sky_strided_mode < 0 && c->stats.samples != 0ull) c->sky_strided = (double)ds.sky_evals < 0.05 * (double)c->stats.samples;
    return RPT_OK;
}

/* rpt_wait: completes everything rpt_render_async enqueued (and folds its stage timing into the statistics). */
int rpt_wait(rpt_ctx *c) {
    if (!c) return RPT_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    /* the last asynchronous batch must have left every slot idle — ALL the context's slots, not only the ones this call used: k_complete's
     * final pass looks at the slots of pixels it could not complete, and a slot beyond this call's n_slots (left by an earlier call with
     * more samples in flight) is outside its view.  One 8-byte read per slot, once per rpt_wait. */
    if (c->async_pending && c->has_state && c->hit.n) {
        const uint32_t all = (uint32_t)c->hit.n;
        k_check_drained<<<rpt_blocks(all), RPT_BLOCK, 0, c->stream>>>(c->hit.p, all, c->dev_stats.p);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (c->async_pending) {
        /* An asynchronous batch runs a fixed number of iterations and never inspects a progress report.  Every batch
         * checks that its predecessor left all slots idle (k_generate_first), the last one is checked just above. */
        c->async_pending = false;
        RPT_TRY(refresh_device_stats(c, "asynchronous batch not drained"));
    }
    c->timing.read_into(c->stats.kernel_ms);
    return RPT_OK;
}

int rpt_stream(rpt_ctx *c, void **stream_out) {
    if (!c || !stream_out) return RPT_EINVAL;
    *stream_out = reinterpret_cast<void *>(c->stream);
    return RPT_OK;
}

/* slots per pixel of THIS call — no more than it has samples for — and the per-slot state at that size.  With moments on at least two: with ONE slot per
 * pixel a sample is accumulated inline by the side stages (k_path.h finish_in_side_stage), which know nothing of the moments record; with two, a one-sample
 * call uses slot 0 of 2 (as a 5-sample call uses 5 of 8) and its sample passes through the completion kernel. */
static int plan_slots(rpt_ctx *c, uint32_t n_samples) {
    uint32_t shift = 0;
    while (shift < c->max_group_shift && (1u << shift) < n_samples) shift += 1;
    if (rpt_lens_active(c) && shift == 0u && c->max_group_shift == 0u) {      /* (as moments below: the side stages restart a path with the reference's camera) */
        c->error = "the camera lens is active and this context keeps one sample of a pixel in flight (rpt_set_samples_in_flight(1), or an image too large for two slots per pixel): "
                   "paths under a lens are started by the completion kernel, which needs at least two; call rpt_set_samples_in_flight(0) or (>= 2), or rpt_set_camera_lens(ctx, NULL)";
        return RPT_EINVAL;
    }
    if (rpt_lens_active(c) && shift == 0u) shift = 1u;
    if (c->moments_on && shift == 0u) {
        if (c->max_group_shift == 0u) {
            c->error = "moments are on and this context keeps one sample of a pixel in flight (rpt_set_samples_in_flight(1), or an image too large for two slots per pixel): "
                       "the moments are added by the completion kernel, which needs at least two; call rpt_set_samples_in_flight(0) or (>= 2), or rpt_set_moments(ctx, 0)";
            return RPT_EINVAL;
        }
        shift = 1u;
    }
    if (c->moments_on && (c->view ? c->view->moments == nullptr : c->moments.n != c->n_pixels)) {      /* (an allocation of the record failed earlier: k_complete_moments must not be launched without it) */
        c->error = "moments are on but their record is not allocated (an earlier allocation failed): call rpt_set_moments(ctx, 0)";
        return RPT_ENOMEM;
    }
    c->group_shift = shift;
    c->n_slots = padded_pixels(c->n_pixels) << shift;
    c->state.group_shift = shift;
    /* samples of one pixel per wave (k_common.h, slot_pix): 1 unless the scene is a large one */
    const uint32_t qs = c->knobs.slot_q_shift >= 0 ? (uint32_t)c->knobs.slot_q_shift : (c->scene.n_triangles >= RPT_BIG_SCENE_TRIANGLES ? 5u : 0u);
    c->state.q_shift = qs < shift ? qs : shift;
    c->state.n_slots = c->n_slots;
    c->queues.sky_wide_limit = std::min(c->n_slots / 16u, c->sky_wide_cfg);   /* the wide sky pass spends 16 threads of the grid per miss */
    HIP_TRY(c, hipSetDevice(c->device));
    return ensure_slot_state(c, c->n_slots, c->cfg.nee_mode != RPT_NEE_NONE, c->cfg.nee_mode == RPT_NEE_MIS);
}

/* waits for the progress report of iteration j: its sky kernel published (j + 1) << 32 | "work remains after iteration j" */
static int await_progress(rpt_ctx *c, uint64_t j, bool &drained) {
    volatile unsigned long long *slot = &c->host_ring.p[j & (RING - 1)];
    unsigned long long v;
    uint64_t spins = 0;
    while (((v = *slot) >> 32) != ((j + 1) & 0xffffffffull)) {
        if (++spins > 2000000000ull || hipStreamQuery(c->stream) == hipSuccess) {
            v = *slot;
            if ((v >> 32) == ((j + 1) & 0xffffffffull)) break;
            HIP_TRY(c, hipGetLastError());
            c->error = "wavefront progress report never arrived (internal error)";
            return RPT_EHIP;
        }
    }
    if ((uint32_t)v == 0u) drained = true;       /* no ray traced, no sample started, no miss waiting: all later iterations are no-ops */
    return RPT_OK;
}

/* what a render call of `iterations` iterations adds to the statistics, enqueued or finished */
static void count_batch(rpt_ctx *c, uint32_t n_samples, uint64_t iterations, uint64_t shade_launches, std::chrono::steady_clock::time_point t0) {
    c->stats.iterations += iterations;
    c->stats.kernel_launches[RPT_STAGE_TRAVERSE] += iterations;
    c->stats.kernel_launches[RPT_STAGE_SHADE] += shade_launches;      /* (one per iteration, but none behind a walk that ended its paths itself) */
    c->stats.kernel_launches[RPT_STAGE_SHADOW] += c->cfg.nee_mode != RPT_NEE_NONE ? iterations : 0;
    c->stats.kernel_launches[RPT_STAGE_SKY] += c->queues.sky_at_end ? 1u : iterations;
    if (!c->view) c->samples += n_samples;        /* (a masked pass: its pixels' own counts move, accum.w and rng.n, not the context's uniform one) */
    c->stats.samples += (uint64_t)c->n_pixels * n_samples;
    c->stats.render_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

/* A masked pass's pixels in place of the context's own for one render call (rpt_ctx.h PixelView): everything the pipeline derives from the pixel count —
 * slots, q-shift, "at least two slots" with moments, known length or polled, implicit_zero, who starts the paths — then follows from the view exactly as
 * it does for a rank that owns few pixels.  The destructor puts the context's own back: every exit path of render_impl passes through it. */
struct ViewScope {
    rpt_ctx *c;
    const uint32_t *pixel_xy;
    uint2 *rng;
    float4 *accum;
    uint32_t n_pixels, max_group_shift, max_slots;
    ViewScope(rpt_ctx *ctx, const PixelView *v) : c(ctx), pixel_xy(ctx->state.pixel_xy), rng(ctx->state.rng), accum(ctx->state.accum), n_pixels(ctx->n_pixels),
                                                  max_group_shift(ctx->max_group_shift), max_slots(ctx->max_slots) {
        if (!v) return;
        c->view = v;
        c->state.pixel_xy = v->pixel_xy; c->state.rng = v->rng; c->state.accum = v->accum; c->state.n_pixels = v->n_pixels;
        c->n_pixels = v->n_pixels;
        c->max_group_shift = v->max_group_shift;
        c->max_slots = padded_pixels(v->n_pixels) << v->max_group_shift;
    }
    ViewScope(const ViewScope &) = delete;
    ~ViewScope() {
        if (!c->view) return;
        c->view = nullptr;
        c->state.pixel_xy = pixel_xy; c->state.rng = rng; c->state.accum = accum; c->state.n_pixels = n_pixels;
        c->n_pixels = n_pixels;
        c->max_group_shift = max_group_shift;
        c->max_slots = max_slots;
    }
};

static int render_impl(rpt_ctx *c, uint32_t n_samples, bool allow_async, const PixelView *view = nullptr) {
    if (!c) return RPT_EINVAL;
    if (!c->has_scene || !c->has_config || !c->has_state) { c->error = "scene, config and reset must precede rpt_render"; return RPT_EINVAL; }
    const ViewScope scope(c, view);
    if (n_samples == 0 || c->n_pixels == 0) { if (!view) c->samples += n_samples; return RPT_OK; }
    if ((uint64_t)n_samples + (1u << c->max_group_shift) >= 0x100000000ull) { c->error = "n_samples too large"; return RPT_EINVAL; }
    RPT_TRY(plan_slots(c, n_samples));
    /* KNOWN LENGTH OR POLLED.  When no slot gets a second sample in this call (n_samples <= slots per pixel) nothing is regenerated: every path
     * ends within max_bounces iterations (lib.rs:62), its misses and shadow rays inside the iteration that produced
     * them (with several slots per pixel a path ended by a side stage is accumulated by the NEXT shade pass: one more
     * iteration) — so exactly that many iterations are enqueued and no progress report is awaited (saves the run-ahead's
     * surplus launches, 4 % of a 1.3 ms batch on 1/8 of an image).  Otherwise (0) the host polls the progress ring. */
    const uint64_t known_iterations =
        (n_samples <= (1u << c->group_shift) && c->queues.sky_threshold <= 1u) ? (uint64_t)c->cfg.c.max_bounces : 0u;
    HIP_TRY(c, hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = c->stream;
    StageTimer &t = c->timing;
    const uint32_t blocks = rpt_blocks(c->n_slots);
    /* asynchronous only when the iteration count is known up front: nothing has to be polled */
    const bool async = allow_async && known_iterations != 0;
    if (!async && c->async_pending) {                     /* the progress ring is about to be reused by the host */
        RPT_TRY(rpt_wait(c));
    }
    if (!async) for (int k = 0; k < RING; ++k) __atomic_store_n(&c->host_ring.p[k], 0ull, __ATOMIC_RELAXED);
    c->call_samples = n_samples;
    /* A miss ends its path (lib.rs:79) and in a batch of known length nothing is started in its place: the misses of all iterations
     * wait in the queue for ONE sky launch after the last iteration (three launches less per batch) */
    c->queues.sky_at_end = known_iterations != 0 ? 1u : 0u;
    c->queues.known_length = known_iterations != 0 ? 1u : 0u;
    /* Without NEE a path's radiance changes only where the path ends, and in a batch of known length no slot owes a second sample (k_path.h first_path_todo is 0
     * for 1 <= n_samples - k <= S): the radiance record of a live path would be sixteen zero bytes.  With several slots per pixel — where a finished sample waits
     * for k_complete — it is not kept: the stages write it only for a path that ends with something added (k_common.h HIT_DONE_ZERO) */
    c->queues.implicit_zero = (known_iterations != 0 && c->cfg.nee_mode == RPT_NEE_NONE && c->group_shift != 0u) ? 1u : 0u;
    /* the shard of the sky queue a slot is pushed into: by its workgroup of the shade stage, whichever variant this call launches */
    c->queues.sky_shard_shift = c->shade_compact ? 11u : 8u;
    static_assert(RPT_BLOCK == 1 << 8 && RPT_BLOCK * RPT_SHADE_ROUNDS == 1 << 11, "sky_shard_shift: slots per workgroup of k_shade");
    t.mark(s, StageTimer::NONE, StageTimer::AT_1);
    /* The stage that opens a render call.  Where the first walk starts the paths itself (an LDS-resident scene, several slots per pixel) it is ONE workgroup
     * that zeroes the call's counters; else a pass over all slots that also writes every slot's camera ray. */
    /* Under an active lens (rpt_set_camera_lens) it is k_generate_lens over all slots: the FIRST walk knows the reference's camera only.  With aperture 0 the
     * rays still share cam_position and iteration 0 stays the FIRST kernel over prepared slots; with an aperture it is the plain walk (launch_iteration). */
    c->first_walk_starts = !rpt_lens_active(c) && rpt_first_walk_starts_paths(c);
    if (rpt_lens_active(c)) rpt_launch_generate_lens(c, n_samples, blocks);
    else k_generate_first<<<c->first_walk_starts ? 1u : blocks, RPT_BLOCK, 0, s>>>(c->state, c->queues, c->cfg, n_samples, c->dev_stats.p, c->first_walk_starts ? 1u : 0u);
    c->stats.kernel_launches[RPT_STAGE_GENERATE] += 1;
    t.mark(s, RPT_STAGE_GENERATE, StageTimer::AT_1);

    /* rpt_debug_short_batch (test aid): enqueue one iteration too few in an asynchronous batch, to prove that the
     * completion checks of rpt_wait / k_generate_first notice */
    const uint64_t planned = known_iterations - (async && known_iterations > 1 && c->test_short_batch ? 1u : 0u);      /* (0: polled) */
    /* generations are completed after every shade stage where slots take more than one sample in this call; a batch of known length completes once, below */
    const bool complete_each = known_iterations == 0 && c->group_shift != 0;
    /* RUN-AHEAD: it only has to cover the enqueue latency (tens of microseconds).  Launches over millions of slots
     * last far longer than that, and every surplus iteration still dispatches its (instantly returning) workgroups. */
    const uint64_t lag = c->n_slots >= (512u << 10) ? 2 : (c->n_slots >= (128u << 10) ? 3 : LAG);
    /* SAFETY NET against a stuck pipeline (a bug), far above the worst case — every sample needs max_bounces iterations, one after
     * another — and above what deferral of sky work can cost */
    const uint64_t it_limit = (uint64_t)n_samples * (uint64_t)(c->cfg.c.max_bounces + 2u) * 16u + 4096u;
    uint64_t it = 0, shade_launches = 0;
    bool drained = c->cfg.c.max_bounces == 0u;
    while (!drained) {
        HIP_TRY_TO(c->error, "hipEventCreate(&e): ", t.take_error());
        shade_launches += dispatch_iteration(c, (uint32_t)it, blocks, complete_each, it + 1 == planned /* (sky_at_end: the one sky launch of the batch) */);
        it += 1;
        if (it == planned) {             /* (no report needed: nothing can be left) */
            /* every path of the batch has ended (max_bounces iterations, side stages included): the one completion of the batch */
            if (c->group_shift != 0) {
                launch_complete(c, (uint32_t)it, 1u);
                c->stats.kernel_launches[RPT_STAGE_COMPLETE] += 1;
                t.mark(s, RPT_STAGE_COMPLETE, StageTimer::AT_1);
            }
            break;
        }
        if (known_iterations == 0 && it >= lag) {
            RPT_TRY(await_progress(c, it - lag, drained));
        }
        if (it > it_limit) { c->error = "wavefront did not drain (internal error)"; return RPT_EHIP; }
    }
    HIP_TRY_TO(c->error, "hipEventCreate(&e): ", t.take_error());
    if (async) {                         /* its stage times are read by rpt_wait */
        c->async_pending = true;
        count_batch(c, n_samples, it, shade_launches, t0);
        return RPT_OK;
    }
    /* a call that enqueued a fixed number of iterations must have left every slot idle: cross-check of that bound */
    if (known_iterations != 0 && c->n_slots && c->group_shift == 0)     /* (several slots per pixel: k_complete's final pass has counted) */
        k_check_drained<<<blocks, RPT_BLOCK, 0, s>>>(c->hit.p, c->n_slots, c->dev_stats.p);
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    count_batch(c, n_samples, it, shade_launches, t0);
    t.read_into(c->stats.kernel_ms);
    /* (an undrained count can only be non-zero for a call that enqueued a fixed number of iterations) */
    return refresh_device_stats(c, "wavefront not drained after its known number of iterations");
}

int rpt_render(rpt_ctx *c, uint32_t n_samples) { return render_impl(c, n_samples, false); }

/* Like rpt_render, but returns as soon as the batch is enqueued when its iteration count is known up front (no slot
 * gets a second sample: n_samples <= slots per pixel); otherwise identical to rpt_render.  Every entry point that
 * reads results synchronises by itself; rpt_wait does so explicitly. */
int rpt_render_async(rpt_ctx *c, uint32_t n_samples) { return render_impl(c, n_samples, true); }

int rpt_read_rng(rpt_ctx *c, rpt_rng_state *out) {
    if (!c || !out) return RPT_EINVAL;
    if (!c->has_state) { c->error = "nothing to read: no config"; return RPT_EINVAL; }
    static_assert(sizeof(rpt_rng_state) == sizeof(uint2), "rpt_read_rng copies the device's uint2 image into the caller's rpt_rng_state");
    return rpt_read_out(c, PixelCopy<uint2>{c->rng.p, nullptr}, out);
}

int rpt_local_pixels(rpt_ctx *c, uint64_t *n) {
    if (!c || !n) return RPT_EINVAL;
    if (!c->has_config) { c->error = "no config"; return RPT_EINVAL; }
    *n = c->n_pixels;
    return RPT_OK;
}

int rpt_set_samples_in_flight(rpt_ctx *c, int s) {
    if (!c) return RPT_EINVAL;
    if (s < 0 || s > (int)RPT_MAX_SAMPLES_IN_FLIGHT) { c->error = "samples in flight must be 0 (automatic) or 1..256"; return RPT_EINVAL; }
    c->samples_in_flight_request = s;
    return reapply_config(c);            /* re-derive the slot count */
}

/* nothing is allocated or invalidated: the mode is read when a batch's shadow stage is enqueued (rpt_traverse.hip launch_shadow) */
int rpt_set_shadow_mode(rpt_ctx *c, uint32_t mode) {
    if (!c) return RPT_EINVAL;
    if (mode != RPT_SHADOW_EXACT && mode != RPT_SHADOW_SEGMENT) { c->error = "rpt_set_shadow_mode: mode must be RPT_SHADOW_EXACT (0) or RPT_SHADOW_SEGMENT (1)"; return RPT_EINVAL; }
    c->shadow_mode = mode;
    return RPT_OK;
}

int rpt_shadow_mode(rpt_ctx *c, uint32_t *mode_out) {
    if (!c || !mode_out) return RPT_EINVAL;
    *mode_out = c->shadow_mode;
    return RPT_OK;
}

int rpt_rank_pixels(rpt_ctx *c, uint32_t rank, uint64_t *n) {
    if (!c || !n) return RPT_EINVAL;
    if (!c->has_config || rank >= c->world) { c->error = "no config / bad rank"; return RPT_EINVAL; }
    std::vector<uint32_t> order;
    rpt_build_pixel_order(c->cfg.c.width, c->cfg.c.height, rank, c->world, order);
    *n = order.size();
    return RPT_OK;
}

int rpt_tile_order(uint32_t width, uint32_t height, uint32_t rank, uint32_t world_size, uint32_t *out_xy, size_t capacity,
                   size_t *n) {
    if (!n || !width || !height || width > 65535u || height > 65535u || !world_size || rank >= world_size) return RPT_EINVAL;
    std::vector<uint32_t> order;
    rpt_build_pixel_order(width, height, rank, world_size, order);
    *n = order.size();
    if (out_xy) {
        if (capacity < order.size()) return RPT_EINVAL;
        memcpy(out_xy, order.data(), order.size() * sizeof(uint32_t));
    }
    return RPT_OK;
}

int rpt_resolve(rpt_ctx *c, uint32_t tonemap_op, float *out_rgb) {
    if (!c || !out_rgb) return RPT_EINVAL;
    if (!c->has_state) { c->error = "nothing to resolve: no config"; return RPT_EINVAL; }
    if (tonemap_op > 6u) { c->error = "tonemap operator must be 0..6"; return RPT_EINVAL; }
    if (c->counts_nonuniform) return rpt_resolve_own(c, tonemap_op, out_rgb);     /* (every pixel by its own accum.w: rpt_adaptive.hip) */
    return rpt_read_out(c, PixelResolve{c->accum.p, (float)c->samples, tonemap_op, nullptr}, out_rgb);
}

int rpt_get_stats(rpt_ctx *c, rpt_stats *out) {
    if (!c || !out) return RPT_EINVAL;
    RPT_TRY(rpt_wait(c));
    DevStats ds;
    HIP_TRY(c, hipMemcpy(&ds, c->dev_stats.p, sizeof(ds), hipMemcpyDeviceToHost));
    std::vector<unsigned long long> shards(RPT_STAT_SHARDS * RPT_STAT_STRIDE, 0ull);
    if (c->ray_shards.p) HIP_TRY(c, hipMemcpy(shards.data(), c->ray_shards.p, shards.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    ds.extension_rays = 0;
    unsigned long long elided = 0ull;
    for (int k = 0; k < RPT_STAT_SHARDS; ++k) { ds.extension_rays += shards[(size_t)k * RPT_STAT_STRIDE]; elided += shards[(size_t)k * RPT_STAT_STRIDE + 1]; }
    c->stats.extension_rays = ds.extension_rays;
    c->stats.shadow_rays = ds.shadow_rays + elided;     /* as the reference counts: one per executed intersect_any (light_pick.rs:141) */
    c->stats.shadow_rays_elided = elided;               /* of those, not walked: their NEE term is zero whatever the walk finds (k_shade.h) */
    c->stats.sky_evals = ds.sky_evals;
    c->stats.light_index_clamped = ds.light_index_clamped;
    *out = c->stats;
    if (ds.undrained != 0ull) { c->error = "a render call found samples still in flight (internal error)"; return RPT_EHIP; }
    return RPT_OK;
}

/* ------------------------------------------------------------ test hooks (include/rpt/rpt_debug.h) -- */
int rpt_debug_short_batch(rpt_ctx *c, int on) {
    if (!c) return RPT_EINVAL;
    c->test_short_batch = on != 0;
    return RPT_OK;
}

}  // extern "C"

/* rpt_adaptive.hip: the batch of a masked pass, on the compact copies of the selected pixels' records */
int rpt_render_view(rpt_ctx *c, uint32_t n_samples, const PixelView *view) { return render_impl(c, n_samples, true, view); }
