/*
 * k_walk_stream.h — what a STREAMED walk kernel needs around the walk of k_walk.h: staging the LDS image, the per-iteration bookkeeping, the workgroup's
 * slot pool, and the measured constants of the LDS-resident (RPT_STREAM_*) and the global-memory (RPT_GSTREAM_*) streamed walks.
 */
#ifndef RPT_K_WALK_STREAM_H
#define RPT_K_WALK_STREAM_H

#include "k_walk.h"

/* Small scenes live in LDS: when the traversal image (SceneViewLds) fits in RPT_LDS_SCENE_BYTES
 * every workgroup copies the upload-time LDS image in once and traverses out of LDS
 * (ds_read_b128, ~64-cycle latency, no pressure on the CU's single vector-memory address
 * unit — the measured limiter once the divisions were gone: ~380 divergent 16-byte
 * wave-loads per wave through one TA per CU).  Larger scenes read through L1/L2. */
extern __shared__ __attribute__((aligned(16))) float4 rpt_lds_dyn[];   /* sized at launch to the scene (LDS variants only) */

template <int THREADS>
__device__ __forceinline__ SceneViewLds stage_scene_lds(const DevScene &sc, float4 *lds_scene, bool shadow_copy = false) {
    const float4 *image = shadow_copy ? sc.lds_image_shadow : sc.lds_image;       /* (the flipped copy: same sizes, same root) */
    for (uint32_t k = threadIdx.x; k < sc.lds_vecs; k += THREADS) lds_scene[k] = image[k];
    __syncthreads();
    return SceneViewLds{lds_scene, sc.lds_pairs, sc.n_triangles, sc.lds_root};
}
template <bool LDS_SCENE, int THREADS>
__device__ __forceinline__ auto stage_scene(const DevScene &sc, float4 *lds_scene) {
    if constexpr (LDS_SCENE) return stage_scene_lds<THREADS>(sc, lds_scene);
    else return SceneViewGlobal{{sc.tri_isect}, sc.nodes};
}

/* Per-iteration bookkeeping that needs no kernel of its own (one thread of the traversal launch).  The shadow queue was
 * consumed by the previous iteration's shadow kernel (same stream).  The sky stage is lazy (k_sky): it drained its queue last
 * iteration only if enough misses had piled up or nothing else was left — the same decision is re-derived here from the same,
 * still unmodified words. */
__device__ __forceinline__ void iteration_bookkeeping(const DevQueues &q, uint32_t iteration) {
    const uint32_t prev = (iteration + 1u) & 1u;
    uint32_t positions, waiting;
    q_extent(q.sky_cnt, positions, waiting);
    q_clear(q.shadow_cnt);
    if (q.sky_at_end == 0u && (waiting >= q.sky_threshold || q.count[Q_ALIVE0 + prev * Q_LINE] == 0u)) q_clear(q.sky_cnt);
    q.count[Q_ALIVE0 + prev * Q_LINE] = 0u;
    q.count[Q_REGEN0 + prev * Q_LINE] = 0u;
}

/* a wave looks for new rays every RPT_STREAM_TRIPS loop trips, once RPT_STREAM_REFILL of its lanes are idle.  Re-measured with 64
 * pixels per wave (round 3, three boxes, DarkCornell Mrays/s relative to 8 / 12): trips 4 / 12 / 16 / 24 / 32: -2.3 / +0.4 / +0.8 /
 * +1.1 / -0.2 %; refill 8 / 16 / 24 at 8 trips: -1 / +-0 / +-0; 16 / 16: +1.1 ... +1.7 % (and +1.1 % with nee = MIS, +1.0 % on 1/8 of
 * the image); 20 / 16 and 24 / 16 the same within noise, 16 / 20 less. */
constexpr int RPT_STREAM_TRIPS = 16;
constexpr int RPT_STREAM_REFILL = 16;
/* The leaf trips of the PLAIN nearest-hit launches (k_walk.h lds_stream_walk_run ONE_TRI, VOTE): one triangle per leaf trip, a lane on a leaf counts double in the
 * vote.  Every other streamed LDS kernel keeps the whole leaf per trip and the plain vote: FIRST's coherent waves lose with short leaf trips
 * (replayed + 8 %, measured + 2.9 %), LAST needs 65 vector registers for them, one more than 8 waves per SIMD leave it, and the shadow kernels have no replay and no
 * A/B of their own. */
constexpr bool RPT_STREAM_PLAIN_ONE_TRI = true;
constexpr int RPT_STREAM_PLAIN_VOTE = 1;
/* The workgroup's pool is one 64-bit LDS word (next slot | end slot << 32): a wave takes slots with ONE 64-bit ds_add that
 * returns a consistent (next, end) pair.  When the span is used up the wave that notices fetches the next span of SPAN
 * slots from the launch-wide counter (one global atomic per SPAN slots) — PERSISTENT workgroups: the grid holds as many
 * workgroups as the GPU keeps resident, and none of them drains before the whole launch runs out of slots.  (Round 1
 * gave every workgroup one fixed span: each of the 4 096 workgroups then ended in its own tail of ever emptier waves —
 * the replay, tools/traversal_sim.py, puts 17 % of the issue slots there — and the launch in a tail of late workgroups.
 * Stealing 512-slot chunks per WAVE from one global counter was measured slower: 65 k atomics per launch on one address.) */
struct WgPool {
    unsigned long long word;     /* lo = next slot, hi = end of the span; hi == 0: the launch has no slots left */
    uint32_t lock;
};
/* the pool word for the span of SPAN slots that starts at g, the value the launch-wide counter returned, in a launch of n slots */
__device__ __forceinline__ unsigned long long wg_pool_span(uint32_t g, uint32_t SPAN, uint32_t n) {
    return g < n ? ((unsigned long long)(g + SPAN < n ? g + SPAN : n) << 32) | g : 0x00000000f0000000ull;
}
/* one lane: take up to `want` slots.  Returns the first slot and how many were obtained (0: none right now);
 * *finished is set once the launch-wide pool is empty. */
__device__ __forceinline__ uint32_t wg_pool_take(WgPool *pool, uint32_t *global_next, uint32_t n_slots, uint32_t SPAN, uint32_t want,
                                                 uint32_t &got, bool &finished) {
    got = 0u;
    for (int attempt = 0; attempt < 4; ++attempt) {
        const unsigned long long v = atomicAdd(&pool->word, (unsigned long long)want);
        const uint32_t next = (uint32_t)v, end = (uint32_t)(v >> 32);
        if (next < end) {
            got = end - next < want ? end - next : want;
            return next;
        }
        if (end == 0u) { finished = true; return 0u; }
        if (atomicCAS(&pool->lock, 0u, 1u) != 0u) return 0u;            /* another wave is fetching the next span: look again later */
        const unsigned long long now = atomicAdd(&pool->word, 0ull);
        if ((uint32_t)now >= (uint32_t)(now >> 32) && (uint32_t)(now >> 32) != 0u) {
            const uint32_t g = atomicAdd(global_next, SPAN);
            atomicExch(&pool->word, wg_pool_span(g, SPAN, n_slots));
        }
        __threadfence_block();
        atomicExch(&pool->lock, 0u);
    }
    return 0u;
}

/* The 1 024-thread workgroups of the streamed LDS walks come two to a CU = 8 waves per SIMD, and that is decided by SGPRs as
 * much as by VGPRs and LDS: a SIMD has 800, a wave is given its count rounded up to 16 plus 16 more the runtime reserves (trap
 * handler), so 8 waves fit only while the kernel needs <= 80.  At 82 the second workgroup no longer fits and the kernel runs at
 * HALF occupancy — which hipModuleOccupancyMaxActiveBlocksPerMultiprocessor does not report (it answers 2) and only the counters
 * show (SQ_WAVE_CYCLES / SQ_BUSY_CYCLES 32 instead of 63).  Measured: the shadow walk 48.3 ms per four batches at 78 SGPRs, 61.2 at
 * 82 (profiles/r03_slp.txt).  So the compiler is held to 80 (it spills nothing: the excess was address arithmetic it can redo). */
#define RPT_LDS_WALK_SGPRS 80

/* ---- streamed walks through GLOBAL memory (scenes too large for LDS) ----------------------------------------
 * Measured on MI355X (profiles/r02base_*): with one ray per lane the global-memory walk runs at 26 % (VeachMIS nearest),
 * 29 % (PBRTest) and 22 % (VeachMIS shadow) lane utilisation while two thirds of its wave cycles wait on L1/L2 — an
 * open scene leaves most slots of a wave without a pending ray after the first bounce (their paths ended in the sky),
 * and any-hit walks end after anything between one and a hundred node visits.  One-wave workgroups make the remedy
 * cheap: a wave owns SPAN consecutive slots (queue entries), and
 *   - (nearest) first compacts the pending ones into a wave-local LDS list — ballot + mbcnt, no atomic, the pool
 *     counter is a scalar register;
 *   - walks with a trip budget and, when RPT_GSTREAM_REFILL lanes are idle, lets them write their results and take
 *     the next rays of the list.
 * Per ray nothing changes (same tests, same order); slots stay identity mapped. */
constexpr int RPT_GSTREAM_RAYS = 8;        /* most slots per lane of a wave (the host lowers it for small launches) */
/* The nearest-hit walk streams better over a longer list — its pending list costs LDS (2 bytes per slot), and LDS is what caps
 * the waves of these kernels, so only where the stack is small: 16 slots per lane with a 16-bit stack of <= 24 entries (3 KB
 * + 2 KB per wave: still 8 waves per SIMD).  Measured, PBRTest traverse per 4 batches: 8 / 12 / 16 / 24 slots per lane
 * 92.9 / 89.0 / 86.9 / 95.1 ms; with a 32-entry stack 16 slots cost (the stand-in 439 -> 468 ms), and the any-hit walk
 * prefers 8 everywhere (VeachMIS shadow 56.6 / 58.0 / 57.6 / 60.8). */
constexpr int RPT_GSTREAM_RAYS_NEAREST_SMALL = 16;
__host__ __device__ constexpr int gstream_rays_nearest(int stack, int width) {
    return (stack <= 24 && width <= 21) ? RPT_GSTREAM_RAYS_NEAREST_SMALL : RPT_GSTREAM_RAYS;
}
constexpr int RPT_GSTREAM_TRIPS = 8;
/* (measured and dropped, round 3: dealing a span's rays grouped by the octant of their direction — the slots of a wave belong to
 * one or two pixels, so after a bounce their rays leave almost one point — 2 M-node stand-in + 2.4 %, PBRTest - 1.3 %, VeachMIS - 0.8 %,
 * the fat-leaf stand-in +- 0) */
constexpr int RPT_GSTREAM_REFILL_FIRST = 64;     /* nearest-hit walk, iteration 0 of a batch: see k_traverse_nearest_gstream */
constexpr int RPT_GSTREAM_REFILL = 24;     /* (round 3, 64 pixels per wave: 8 / 16 / 24 idle lanes: PBRTest 7 390 / 7 390 / 7 445, VeachMIS 6 560 / 6 615 / 6 655 Mrays/s;
                                              trips 4 / 8 / 12 / 16: 7 355 / 7 390 / 7 320 / 7 250 and 6 620 / 6 615 / 6 530 / 6 480) */
/* The global-memory walks wait on memory two thirds of their cycles (profiles/r02_*_pmc_sq.txt) and live on occupancy.  Left
 * alone the compiler settles at 68 / 77 VGPRs (7 / 6 waves per SIMD); asked for 8 it needs 57 / 58 and spills nothing:
 * PBRTest traverse 97.3 -> 92.8 ms per 4 batches, VeachMIS traverse + shadow 91.8 -> 87.9, the 1 M-triangle stand-in's
 * shadow stage 391 -> 366.  (Wider stack entries cap the occupancy through LDS instead: hence the 24-bit form, WaveStack.) */
constexpr int RPT_GSTREAM_WAVES = 8;
constexpr int RPT_GSTREAM_WAVES_COOP = 8;  /* the fat-leaf build holds a leaf's triangle records in registers: 63 / 64 VGPRs, no spill.  Requesting the NEXT
                                              leaf's records one leaf ahead (9 more registers) was measured and lost at every occupancy: the 1 M-triangle
                                              stand-in 2 343 Mrays/s without, 2 008 / 2 164 / 2 099 with it at 8 (spilling) / 7 / 6 waves per SIMD */
__host__ __device__ constexpr int gstream_waves(int stack, int width, bool coop) {
    return (width <= 21 || (width == 24 && stack <= 24)) ? (coop ? (width >= 21 ? 7 : RPT_GSTREAM_WAVES_COOP) : RPT_GSTREAM_WAVES) : 1;   /* (where LDS allows it at all;
                                                             fat leaves + 21-bit entries: 8 waves would spill 18 registers, + 24-bit entries: 3) */
}
/* (8 waves per SIMD also need <= 80 SGPRs, see RPT_LDS_WALK_SGPRS: the builds the shipped scenes and the stand-ins use have 78; some of the
 * others — 21- and 32-bit stack entries — have 81 and run 7.  amdgpu_num_sgpr takes a literal, not a template expression, so it cannot follow
 * gstream_waves.) */
/* XCD-aware span mapping was measured on these kernels and rejected (profiles/r03_deepbvh_experiments.txt): workgroup id i runs on XCD
 * i % 8, so span = id spreads neighbouring pixels over all eight L2s.  Giving each XCD one contiguous eighth of the launch: 2 x
 * SLOWER on the 1 M-triangle stand-in (the XCD that owns the expensive part of the image finishes alone); runs of 64 consecutive
 * spans per XCD inside groups of 512: +-0; runs of 512: -14 %.  The identity mapping stays. */

#endif /* RPT_K_WALK_STREAM_H */
