/*
 * rpt_traverse.hip — the traversal stages of librpt_hip.so: which kernel of k_traverse.h walks the extension rays / the shadow rays of a context's scene,
 * and on which grid.  Its own translation unit since round 6 (the walk kernels are half of the library's compile time; the three units build in parallel).
 * Entry points (rpt_ctx.h): rpt_launch_nearest, rpt_first_walk_starts_paths, rpt_launch_shadow, rpt_launch_trace_debug, rpt_last_walk_attributes.
 */
#include <hip/hip_runtime.h>

#include <type_traits>

#include "rpt_ctx.h"
#include "k_traverse.h"

namespace {

constexpr int GLOBAL_THREADS = 64;   /* workgroup size of the one-ray-per-lane global-memory walks.  One wave: no scene staging to share, and a
                                        finished wave frees its stack at once (PBRTest traverse -5 %) */
/* workgroup size of the LDS-resident-scene traversal kernels: 2 x (32 KB of 16-bit stacks + up to 32 KB of scene = the 64 KB a
 * workgroup may hold) per CU = 32 waves */
constexpr int LDS_THREADS = 1024;


template <int STACK>
static int gstream_stack_width(const rpt_ctx *c) {
    /* An entry is a node index, so its width follows the POOL's size, not the tree's depth (a shallow tree may sit in a sparse pool).  The 16-entry stack is
     * given only to pools of fewer than 65 536 nodes (rpt_scene.hip, where stack_cap is set); a pair-shaped pool links to no index from 2^24 on
     * (pool_is_pair_shaped), so the 24 bits that the 24-entry stack stops at hold every entry whatever the node count.  RPT_STACK_BITS, a test aid, widens
     * the entries of deep trees. */
    if (STACK == 16) return 16;
    const int bits = c->knobs.stack_bits;
    const int w = (c->scene.n_nodes < 65536u && bits <= 16) ? 16 : (c->scene.n_nodes < (1u << 21) && bits <= 21) ? 21 : (c->scene.n_nodes < (1u << 24) && bits <= 24) ? 24 : 32;
    return STACK == 24 && w > 24 ? 24 : w;
}
/* launch(std::integral_constant<int, WIDTH>) for the entry width gstream_stack_width<STACK> returned: only the (STACK, WIDTH) pairs it can return
 * are instantiated */
template <int STACK, typename F>
static void with_stack_width(int width, F &&launch) {
    if constexpr (STACK == 16) launch(std::integral_constant<int, 16>{});
    else if (width == 16) launch(std::integral_constant<int, 16>{});
    else if (width == 21) launch(std::integral_constant<int, 21>{});
    else if constexpr (STACK == 24) launch(std::integral_constant<int, 24>{});
    else if (width == 24) launch(std::integral_constant<int, 24>{});
    else launch(std::integral_constant<int, 32>{});
}
/* slots per wave of the streamed global-memory walks: as many as keep >= gstream_min_waves waves in the launch, at most `most` per lane */
static uint32_t gstream_span(const rpt_ctx *c, uint32_t most) {
    const uint32_t wanted = c->n_slots / (c->gstream_min_waves * RPT_WAVE);
    const uint32_t g = wanted < 1u ? 1u : (wanted > most ? most : wanted);
    return g * RPT_WAVE;
}
/* spans of the streamed LDS walks: persistent workgroups (as many as stay resident: 2 per CU) fetch spans of slots from a launch-wide counter; a span = 1/32 of a
 * workgroup's share, between 1 and 8 slots per lane (measured at 33 M slots: 8192 / 4096 / 2048 / 1024 slots per span: DarkCornell 9 995 / 10 160 / 10 255 / 10 200
 * Mrays/s with 64 pixels per wave; rounds 1-2, two pixels per wave, preferred 4096) */
static uint32_t lds_stream_span(const rpt_ctx *c, uint32_t &grid) {
    const uint32_t wgs = c->stream_max_blocks;
    uint32_t span = c->n_slots / (wgs * 32u);
    span = span < (uint32_t)LDS_THREADS ? (uint32_t)LDS_THREADS : (span > 8u * LDS_THREADS ? 8u * LDS_THREADS : span);
    span = (span + LDS_THREADS - 1) / LDS_THREADS * LDS_THREADS;
    const uint32_t n_spans = (c->n_slots + span - 1) / span;
    grid = n_spans < wgs ? n_spans : wgs;
    return span;
}

/* the streamed global-memory nearest-hit walk for the (stack capacity, entry width) pairs a scene can have */
template <int STACK, bool COOP>
static void launch_nearest_gstream(rpt_ctx *c, uint32_t iteration) {
    const int width = gstream_stack_width<STACK>(c);
    const uint32_t span = gstream_span(c, (uint32_t)gstream_rays_nearest(STACK, width)), blocks = (c->n_slots + span - 1) / span;
    with_stack_width<STACK>(width, [&](auto W) {
        k_traverse_nearest_gstream<STACK, decltype(W)::value, COOP><<<blocks, RPT_WAVE, 0, c->stream>>>(c->scene, c->state, c->queues, iteration, span);
    });
}

/* The nearest-hit traversal stage for the context's scene and state: which kernel, which grid.  Used by every iteration of a
 * render call and by rpt_debug_trace_rays_production (per-ray parity of exactly these kernels).
 *   a scene whose traversal image lives in LDS : the persistent streamed LDS walk (FIRST: camera rays; LAST: the last rays of a batch without NEE)
 *   a pair-shaped node pool (every pool the reference's builder makes)  : the streamed global-memory walk over pair records
 *   any other tree (a foreign builder's pool)  : the generic one-ray-per-lane walk over the uploaded nodes */
/* Returns true when the launch ENDS the paths it walked (the LAST walk with several slots per pixel: no shade launch follows it). */
template <int STACK>
bool launch_nearest(rpt_ctx *c, uint32_t iteration, bool last_without_nee = false /* the last extension rays of a batch of known length, no NEE */,
                    bool camera_rays = false /* iteration 0 of a render call: every ray leaves cfg.cam_position */,
                    bool start_paths = false /* camera_rays, and the slots were NOT prepared by k_generate_first: rpt_first_walk_starts_paths */) {
    hipStream_t s = c->stream;
    DevStats *stats = c->dev_stats.p;
    if (STACK == 16 && c->scene.lds_scene) {
        const size_t lds_bytes = (size_t)c->scene.lds_vecs * sizeof(float4);
        uint32_t grid;
        const uint32_t span = lds_stream_span(c, grid);
        const float *cam = c->cfg.c.cam_position;
        if (last_without_nee && c->scene.last_emit_n <= RPT_LAST_EMIT_MAX) {
            k_traverse_nearest_stream<16, LDS_THREADS, RPT_NEAREST_LAST><<<grid, LDS_THREADS, lds_bytes + (size_t)c->scene.last_flip_vecs * sizeof(float4), s>>>(c->scene, c->state, c->queues, iteration, span, 0.0f, 0.0f, 0.0f, c->cfg, 0u, stats);
            return c->queues.implicit_zero != 0u;            /* (the kernel's done_here: last_without_nee and several slots per pixel) */
        }
        if (camera_rays)
            k_traverse_nearest_stream<16, LDS_THREADS, RPT_NEAREST_FIRST><<<grid, LDS_THREADS, lds_bytes, s>>>(c->scene, c->state, c->queues, iteration, span, cam[0], cam[1], cam[2], c->cfg, start_paths ? c->call_samples : 0u, stats);
        else k_traverse_nearest_stream<16, LDS_THREADS><<<grid, LDS_THREADS, lds_bytes, s>>>(c->scene, c->state, c->queues, iteration, span, 0.0f, 0.0f, 0.0f, c->cfg, 0u, stats);
    } else if (c->scene.gpairs) {
        if (c->fat_leaves) launch_nearest_gstream<STACK, true>(c, iteration);
        else launch_nearest_gstream<STACK, false>(c, iteration);
    } else {
        const uint32_t nb = (c->n_slots + GLOBAL_THREADS - 1) / GLOBAL_THREADS;
        k_traverse_nearest<32, GLOBAL_THREADS><<<nb, GLOBAL_THREADS, 0, s>>>(c->scene, c->state, c->queues, iteration);
    }
    return false;
}

/* the streamed global-memory any-hit walk (FIXED: over the flipped copy, left child first — shadow_order.h; the `_seg` twins: the context is in
 * RPT_SHADOW_SEGMENT mode, k_walk.h shadow_segment_bound) */
template <int STACK, bool COOP>
static void launch_shadow_gstream(rpt_ctx *c, uint32_t q_positions) {
    const int width = gstream_stack_width<STACK>(c);
    const uint32_t span = gstream_span(c, (uint32_t)RPT_GSTREAM_RAYS), blocks = (q_positions + span - 1) / span;
    const bool segment = c->shadow_mode == RPT_SHADOW_SEGMENT;
    with_stack_width<STACK>(width, [&](auto W) {
        constexpr int WIDTH = decltype(W)::value;
        if (segment) {
            if (c->scene.gpairs_shadow) k_traverse_shadow_gstream_seg<STACK, WIDTH, COOP, true><<<blocks, RPT_WAVE, 0, c->stream>>>(c->scene, c->state, c->queues, c->cfg, c->dev_stats.p, span);
            else k_traverse_shadow_gstream_seg<STACK, WIDTH, COOP, false><<<blocks, RPT_WAVE, 0, c->stream>>>(c->scene, c->state, c->queues, c->cfg, c->dev_stats.p, span);
        } else if (c->scene.gpairs_shadow) k_traverse_shadow_gstream<STACK, WIDTH, COOP, true><<<blocks, RPT_WAVE, 0, c->stream>>>(c->scene, c->state, c->queues, c->cfg, c->dev_stats.p, span);
        else k_traverse_shadow_gstream<STACK, WIDTH, COOP, false><<<blocks, RPT_WAVE, 0, c->stream>>>(c->scene, c->state, c->queues, c->cfg, c->dev_stats.p, span);
    });
}


template <int STACK>
void launch_shadow(rpt_ctx *c) {
    hipStream_t s = c->stream;
    const size_t lds_bytes = (size_t)c->scene.lds_vecs * sizeof(float4);
    const uint32_t q_positions = c->n_slots + RPT_Q_SLACK, blocks_q = (q_positions + RPT_BLOCK - 1) / RPT_BLOCK;
    const bool segment = c->shadow_mode == RPT_SHADOW_SEGMENT;      /* read here, at enqueue: rpt_set_shadow_mode holds from the next batch on */
    if (STACK == 16 && c->scene.lds_scene) {
        uint32_t grid;
        const uint32_t span = lds_stream_span(c, grid);
        if (segment) {
            if (c->scene.lds_image_shadow) k_traverse_shadow_stream_seg<16, LDS_THREADS, true><<<grid, LDS_THREADS, lds_bytes, s>>>(c->scene, c->state, c->queues, c->dev_stats.p, span);
            else k_traverse_shadow_stream_seg<16, LDS_THREADS, false><<<grid, LDS_THREADS, lds_bytes, s>>>(c->scene, c->state, c->queues, c->dev_stats.p, span);
        } else if (c->scene.lds_image_shadow) k_traverse_shadow_stream<16, LDS_THREADS, true><<<grid, LDS_THREADS, lds_bytes, s>>>(c->scene, c->state, c->queues, c->dev_stats.p, span);
        else k_traverse_shadow_stream<16, LDS_THREADS, false><<<grid, LDS_THREADS, lds_bytes, s>>>(c->scene, c->state, c->queues, c->dev_stats.p, span);
        k_shadow_resolve<<<blocks_q, RPT_BLOCK, 0, s>>>(c->state, c->queues, c->cfg);
    } else if (c->scene.gpairs) {
        if (c->fat_leaves) launch_shadow_gstream<STACK, true>(c, q_positions);
        else launch_shadow_gstream<STACK, false>(c, q_positions);
    } else {
        const uint32_t nb = (q_positions + GLOBAL_THREADS - 1) / GLOBAL_THREADS;
        if (segment) k_traverse_shadow_seg<32, GLOBAL_THREADS><<<nb, GLOBAL_THREADS, 0, s>>>(c->scene, c->state, c->queues, c->cfg, c->dev_stats.p);
        else k_traverse_shadow<32, GLOBAL_THREADS><<<nb, GLOBAL_THREADS, 0, s>>>(c->scene, c->state, c->queues, c->cfg, c->dev_stats.p);
    }
}

}  // namespace

bool rpt_launch_nearest(rpt_ctx *c, uint32_t iteration, bool last_without_nee, bool camera_rays, bool start_paths) {
    switch (c->stack_cap) {
        case 16: return launch_nearest<16>(c, iteration, last_without_nee, camera_rays, start_paths);
        case 24: return launch_nearest<24>(c, iteration, last_without_nee, camera_rays, start_paths);
        default: return launch_nearest<32>(c, iteration, last_without_nee, camera_rays, start_paths);
    }
}

/* the walk of a render call's iteration 0 is the FIRST kernel and can start the call's first paths itself: an LDS-resident scene, several slots per pixel
 * (with one, k_generate_first is also where max_bounces == 0 and the in-place restarts are handled) and at least one bounce */
bool rpt_first_walk_starts_paths(const rpt_ctx *c) {
    return c->stack_cap == 16 && c->scene.lds_scene != 0u && c->state.group_shift != 0u && c->cfg.c.max_bounces != 0u;
}

void rpt_launch_shadow(rpt_ctx *c) {
    switch (c->stack_cap) {
        case 16: launch_shadow<16>(c); break;
        case 24: launch_shadow<24>(c); break;
        default: launch_shadow<32>(c); break;
    }
}

hipError_t rpt_last_walk_attributes(hipFuncAttributes *out) {
    return hipFuncGetAttributes(out, reinterpret_cast<const void *>(&k_traverse_nearest_stream<16, LDS_THREADS, RPT_NEAREST_LAST>));
}

/* rpt_debug_trace_rays: plain ray arrays through the reference-order walk (traverse_one), out of LDS where the scene lives there
 * (any_hit 2: the segment-bounded any-hit walk) */
void rpt_launch_trace_debug(rpt_ctx *c, int any_hit, uint32_t n, const float *o, const float *d, const float *max_t, float *out_t, uint32_t *out_tri, uint32_t *out_flags) {
    hipStream_t s = c->stream;
    if (c->stack_cap == 16 && c->scene.lds_scene) {
        const unsigned bl = (n + LDS_THREADS - 1) / LDS_THREADS;
        const size_t lds_bytes = (size_t)c->scene.lds_vecs * sizeof(float4);
        if (any_hit == 2) k_trace_debug_seg<16, true, true, LDS_THREADS><<<bl, LDS_THREADS, lds_bytes, s>>>(c->scene, n, o, d, max_t, out_t, out_tri, out_flags);
        else if (any_hit) k_trace_debug<16, true, true, LDS_THREADS><<<bl, LDS_THREADS, lds_bytes, s>>>(c->scene, n, o, d, max_t, out_t, out_tri, out_flags);
        else k_trace_debug<16, false, true, LDS_THREADS><<<bl, LDS_THREADS, lds_bytes, s>>>(c->scene, n, o, d, max_t, out_t, out_tri, out_flags);
    } else {
        const unsigned blocks = (n + RPT_BLOCK - 1) / RPT_BLOCK;
        if (any_hit == 2) k_trace_debug_seg<32, true, false, RPT_BLOCK><<<blocks, RPT_BLOCK, 0, s>>>(c->scene, n, o, d, max_t, out_t, out_tri, out_flags);
        else if (any_hit) k_trace_debug<32, true, false, RPT_BLOCK><<<blocks, RPT_BLOCK, 0, s>>>(c->scene, n, o, d, max_t, out_t, out_tri, out_flags);
        else k_trace_debug<32, false, false, RPT_BLOCK><<<blocks, RPT_BLOCK, 0, s>>>(c->scene, n, o, d, max_t, out_t, out_tri, out_flags);
    }
}
