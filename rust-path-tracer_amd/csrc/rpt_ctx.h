/*
 * rpt_ctx.h — the context object behind the C ABI of include/rpt/rpt.h, shared by the translation units of
 * librpt_hip.so (rpt_hip.hip: life cycle, state and wavefront scheduling; rpt_scene.hip: scene preparation; rpt_traverse.hip: the traversal stages;
 * rpt_comm.hip: multi-GPU gather over RCCL, read-back; rpt_denoise.hip: guide buffers and the denoise filter; rpt_moments.hip: sample moments, noise estimate,
 * render to a noise target; rpt_adaptive.hip: masked passes over chosen pixels, per-pixel counts to a noise target; rpt_models.hip: material models and the
 * shade stage's models variant; rpt_lens.hip: the thin-lens camera and the kernels that start paths through it; rpt_debug.hip: test hooks).  k_image_order.h: the one kernel and the one read-out routine that turn the tile-major pixel order
 * into a row-major image, for every unit that hands one to the caller.
 */
#ifndef RPT_CTX_H
#define RPT_CTX_H

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rpt/rpt.h"
#include "../../include/rpt/rpt_debug.h"
#include "k_common.h"
#include "shadow_order.h"

/* on failure of `expr`: `dest` = prefix + the HIP error, return RPT_EHIP (dest: the context's error, rpt_create_error() or a string of one call) */
#define HIP_TRY_TO(dest, prefix, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { (dest) = std::string(prefix) + hipGetErrorString(e_); return RPT_EHIP; } } while (0)
#define HIP_TRY(ctx, expr) HIP_TRY_TO((ctx)->error, #expr ": ", expr)
/* an RPT_* code other than RPT_OK from `expr` (which has stated the error itself) ends the caller with it */
#define RPT_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

/* device (hipMalloc) or pinned host (hipHostMalloc, with its flags) memory */
struct DeviceMem {
    static hipError_t get(void **p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
    static void put(void *p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t get(void **p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
    static void put(void *p) { (void)hipHostFree(p); }
};

/* `n` elements of T that the buffer owns: freed by its destructor, by `release` or by the next `alloc` (which frees BEFORE it allocates, so a
 * resize never holds both; a failed or empty alloc leaves p == nullptr, n == 0); move-only */
template <typename T, typename Mem> struct OwnedBuf {
    T *p = nullptr;
    size_t n = 0;
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    OwnedBuf(OwnedBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), n(std::exchange(o.n, 0)) {}
    OwnedBuf &operator=(OwnedBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            n = std::exchange(o.n, 0);
        }
        return *this;
    }
    ~OwnedBuf() { release(); }
    hipError_t alloc(size_t count, unsigned flags = 0) {
        release();
        if (!count) return hipSuccess;
        const hipError_t e = Mem::get(reinterpret_cast<void **>(&p), count * sizeof(T), flags);
        if (e != hipSuccess) p = nullptr;
        else n = count;
        return e;
    }
    /* alloc(count) + the copy of that many elements' bytes from host memory (complete when it returns) */
    hipError_t from_host(const void *src, size_t count) {
        const hipError_t e = alloc(count);
        return e != hipSuccess || !count ? e : hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
    }
    void release() {
        if (p) Mem::put(p);
        p = nullptr;
        n = 0;
    }
};
template <typename T> using DevBuf = OwnedBuf<T, DeviceMem>;
template <typename T> using PinnedBuf = OwnedBuf<T, PinnedMem>;

/* workgroups of RPT_BLOCK threads that cover n items */
constexpr unsigned rpt_blocks(size_t n) { return (unsigned)((n + RPT_BLOCK - 1) / RPT_BLOCK); }

/* ONE device allocation carved up 256-byte aligned: hipMalloc / hipFree cost 0.1-0.3 ms each, so a call that needs many scratch buffers takes them from one */
struct Arena {
    DevBuf<unsigned char> mem;
    size_t used = 0;
    static size_t pad(size_t bytes) { return (bytes + 255u) & ~(size_t)255u; }
    hipError_t reserve(size_t bytes) { used = 0; return mem.alloc(bytes); }
    template <typename T> T *take(size_t count) { T *p = reinterpret_cast<T *>(mem.p + used); used += pad(count * sizeof(T)); return p; }
};

/* RPT_STAGE_TIMING: HIP events between the stage kernels, read into rpt_stats.kernel_ms once the stream has been drained.  Every event is recorded
 * together with the stage that the time SINCE THE PREVIOUS EVENT belongs to (NONE: a starting mark, the time before it is nobody's), so reading them is one
 * loop over consecutive pairs whatever the level, the number of iterations, and whether one batch or several asynchronous ones were recorded.  A mark names
 * the levels it is taken at: level 1 = after every stage kernel, level 2 = only around the traversal kernel.  The events are the timer's own: read ones are
 * kept for the next batch, all are destroyed with it — while the context's device is current (rpt_destroy calls clear() itself, before it destroys the stream). */
struct StageTimer {
    static constexpr int NONE = -1, AT_1 = 1, AT_2 = 2;
    struct Mark { hipEvent_t event; int stage; };
    int level = 0;                              /* 0 off, AT_1, AT_2 */
    std::vector<Mark> recorded;                 /* not read yet, in stream order */
    std::vector<hipEvent_t> idle;
    hipError_t create_error = hipSuccess;       /* a failed hipEventCreate: marks stop until take_error() has reported it */
    StageTimer() = default;
    StageTimer(const StageTimer &) = delete;             /* (the events have one owner) */
    ~StageTimer() { clear(); }
    void mark(hipStream_t stream, int stage, int levels) {
        if ((levels & level) == 0 || create_error != hipSuccess) return;
        hipEvent_t e;
        if (idle.empty()) { if ((create_error = hipEventCreate(&e)) != hipSuccess) return; }
        else { e = idle.back(); idle.pop_back(); }
        (void)hipEventRecord(e, stream);
        recorded.push_back(Mark{e, stage});
    }
    hipError_t take_error() { return std::exchange(create_error, hipSuccess); }
    /* after the stream has been synchronised */
    void read_into(double *kernel_ms) {
        float ms;
        for (size_t k = 0; k < recorded.size(); ++k) {
            if (k != 0 && recorded[k].stage != NONE && hipEventElapsedTime(&ms, recorded[k - 1].event, recorded[k].event) == hipSuccess) kernel_ms[recorded[k].stage] += ms;
            idle.push_back(recorded[k].event);
        }
        recorded.clear();
    }
    void clear() {
        for (const Mark &m : recorded) (void)hipEventDestroy(m.event);
        for (hipEvent_t e : idle) (void)hipEventDestroy(e);
        recorded.clear(); idle.clear();
    }
};

constexpr int RPT_RING_LAG = 6;   /* most iterations the host may run ahead of the progress report it inspects (small launches) */
constexpr int RPT_RING = 16;      /* power of two, > RPT_RING_LAG */

/* one history slot of rpt_denoise_temporal (k_temporal.h): 56 bytes per pixel, row-major, and the view it was made under */
struct TemporalSlot {
    DevBuf<float4> h, g0, g1;             /* (e_h | N), and copies of the guide records (normal | depth), (position | kind bits) */
    DevBuf<float2> mu;                    /* (mu1, mu2) */
    float ro[3] = {0.0f, 0.0f, 0.0f}, euler[9] = {};   /* that view's camera position and DevConfig::euler */
    uint64_t epoch = 0;                   /* rpt_ctx::accum_epoch of the call that wrote it */
    bool demodulated = false;             /* e_h is divided by the albedo */
    bool valid = false;
    void release() { h.release(); g0.release(); g1.release(); mu.release(); valid = false; }
};

/* rpt_denoise.hip: what rpt_denoise / rpt_read_guides keep on a context — allocated on first use, released on destroy and on a resize.  The guides
 * belong to (scene, configuration): rpt_upload_scene and rpt_set_config mark them stale, the next use rebuilds them. */
struct DenoiseState {
    DevBuf<float4> g0, g1, albedo;        /* row-major W x H: (normal | depth), (position | kind bits), (albedo | -) */
    DevBuf<float4> ping, pong;            /* the two images the passes alternate between */
    DevBuf<float> rgb;                    /* W x H x 3: the result, before it leaves the device */
    DevBuf<float> variance;               /* W x H: the variance plane of rpt_denoise_variance (allocated by its first call) */
    DevBuf<float4> moments_in;            /* W x H, row-major: a caller's moments image, uploaded per call of rpt_denoise_variance (allocated by the first such call) */
    DevBuf<uint32_t> order;               /* x | y << 16 of every pixel of the image in tile order (rank 0 of 1): a wave of guide rays is an 8 x 8 block */
    uint32_t width = 0, height = 0;       /* what the buffers are sized for */
    bool guides_valid = false;
    uint32_t through_glass = 0;           /* rpt_set_guides_through_glass: the budget of interfaces K (k_guides_glass.h); 0: first-hit guides */
    rpt_guides_info info = {};            /* the last build, for rpt_guides_info_get (max_interfaces is filled in when asked) */
    /* rpt_denoise_temporal (k_temporal.h): the two history slots, allocated at its first use, freed by rpt_temporal_reset, a resize and destroy */
    TemporalSlot last, previous;          /* what the most recent call produced; the history from before the current accumulator epoch */
    DevBuf<float> history_t;              /* W x H: T per pixel, before it leaves the device */
    DevBuf<uint32_t> inverse;             /* W x H: the element of `order` that is row-major pixel i (the fused kernel reads the tile-major accumulator by rows) */
    DevBuf<unsigned long long> with_history;   /* the kernel's count of pixels that reused history */
    DevBuf<unsigned long long> clamped;   /* the firefly clamp's count of clamped pixels (k_firefly.h; allocated by the first call with the clamp on) */
    bool scene_changed = false;           /* rpt_upload_scene since the last call of rpt_denoise_temporal: that call drops the history */
    bool history_dropped = false;         /* a resize freed a valid history: the next call reports it */
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   /* guides begin / end, filter begin / end (created with the buffers, destroyed by rpt_denoise_release) */
};

struct rpt_comm;                  /* rpt_comm.hip: RCCL communicator + gather buffers of one context */

/* The pixels a render call works on when they are not the context's own: the compact copies a masked pass made of the selected pixels' records
 * (rpt_adaptive.hip).  render_impl (rpt_hip.hip) swaps them in for the call — state.{pixel_xy, rng, accum, n_pixels}, n_pixels, the moments record the
 * completion kernel and plan_slots look at, max_group_shift / max_slots — and puts the context's own back on every exit path. */
struct PixelView {
    const uint32_t *pixel_xy;
    uint2 *rng;
    float4 *accum;
    float4 *moments;                      /* null unless moments are on */
    uint32_t n_pixels;
    uint32_t max_group_shift;             /* log2 of the most slots per pixel the view may keep busy (rpt_adaptive.hip view_max_shift) */
};

/* rpt_adaptive.hip: what masked passes keep on a context — allocated at first use, grown and never shrunk, released with the pixel state and on destroy */
struct AdaptiveState {
    DevBuf<uint8_t> mask, flags;          /* the caller's row-major mask as uploaded; one flag byte per owned pixel */
    DevBuf<uint32_t> wg_count, wg_offset; /* flagged pixels per workgroup of 256 pixels, and their exclusive scan */
    DevBuf<unsigned long long> result;    /* an AdResult (k_adaptive.h): n_active, the noise counts, the range of m.z */
    DevBuf<uint32_t> active, pixel_xy;    /* the compact arrays: active[i] = the pixel entry i came from, and the copies of its records */
    DevBuf<uint2> rng;
    DevBuf<float4> accum, moments;
    DevBuf<uint32_t> tiles;               /* the window rule (k_adaptive.h k_ad_window): one AdTile of 4 words per owned tile, rpt_build_tile_table for tiles_key */
    uint64_t tiles_key = 0;               /* width | height << 16 | rank << 32 | world << 48 the table was built for (0: none) */
    uint32_t n_tiles = 0;
    uint32_t n_active = 0;                /* of the last selection read (rpt_adaptive_selected): what the next pass gathers */
    void release() {
        mask.release(); flags.release(); wg_count.release(); wg_offset.release(); result.release();
        tiles.release(); tiles_key = 0; n_tiles = 0;
        active.release(); pixel_xy.release(); rng.release(); accum.release(); moments.release();
    }
};

/* Every environment variable the library reads, read in ONE place (rpt_read_knobs, rpt_hip.hip; rpt_create copies them into the context).  None changes
 * a result (tests/test_gpu_parity.py::test_developer_knobs_do_not_change_the_image); they exist for tests that must reach a code path a shipped scene
 * does not take, and for the bench's stage timing.  Rounds 1-5 had thirty — every A/B of a tuning round left one behind, with the losing code path kept alive
 * behind it; round 6 removed the knobs whose alternative lost with kept evidence (one-shot walks instead of the streamed ones, per-iteration sky
 * launches in batches of known length, deferred sky threshold, span / grid sizes of the streamed walks, IEEE-only division, ...) together with that code. */
struct rpt_knobs {
    int stage_timing = 0;             /* RPT_STAGE_TIMING    1: HIP events after every stage kernel (rpt_stats.kernel_ms); 2: around the traversal kernel only */
    bool upload_timing = false;       /* RPT_UPLOAD_TIMING   1: section times of rpt_upload_scene / rpt_bvh_build_gpu on stderr */
    int slot_q_shift = -1;            /* RPT_SLOT_Q_SHIFT    0..5: log2 of the samples of a pixel that share a wave (automatic: 5 for scenes of 2^19 triangles and more) */
    int shadow_order = -1;            /* RPT_SHADOW_ORDER    near | fixed: the any-hit walks' order instead of the probe's choice (shadow_order.h) */
    int last_order = -1;              /* RPT_LAST_ORDER      off | near | opaque | small | ratio: the last extension rays' walk instead of the probe's choice */
    int shade_compact = -1;           /* RPT_SHADE_COMPACT   0 | 1: the packed shade stage off / on instead of by the scene's own miss share */
    int sky_strided = -1;             /* RPT_SKY_STRIDED     0: one thread per queued miss; N >= 1: the strided sky stage (N > 1: with a grid of N workgroups) */
    int stack_bits = 16;              /* RPT_STACK_BITS      16 | 21 | 24 | 32: narrowest stack entry of the streamed global-memory walks (deep trees only) */
    int coop_leaves = -1;             /* RPT_COOP_LEAVES     0 | 1: the wave-cooperative leaf build of the streamed walks off / on instead of by leaf size */
    bool no_lds_scene = false;        /* RPT_NO_LDS_SCENE    1: walk a scene that would fit in LDS from global memory */
    int bvh_team_min = 0;             /* RPT_BVH_TEAM_MIN    rpt_bvh_build_gpu: smallest node split by a team of workgroups (0: the built-in threshold) */
    /* (RPT_RCCL_LIBRARY — the collective library to dlopen instead of librccl.so, test stand-in only — is read by rpt_comm.hip when the first communicator is made) */
};
rpt_knobs rpt_read_knobs();

struct rpt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string error;
    uint32_t rank = 0, world = 1;
    rpt_knobs knobs;                     /* copy of rpt_read_knobs() at rpt_create */
    bool shade_compact = false;          /* shade stage variant in use: traversed slots packed per workgroup before shading (k_shade<.., COMPACT>) */
    int shade_compact_mode = -1;         /* -1 automatic (refresh_device_stats), 0 / 1 forced by RPT_SHADE_COMPACT */
    double shade_compact_at = 0.7;       /* automatic: on when more than this share of the samples ends in the sky */
    bool fat_leaves = false;             /* some leaf holds more than RPT_COOP_LEAF_MIN triangles: the streamed walks' wave-cooperative build
                                            (RPT_COOP_LEAVES=0/1 forces the other build for tests; both give the same image) */
    uint32_t gstream_min_waves = 32768;
    uint32_t stream_max_blocks = 512;    /* persistent workgroups of the streamed LDS traversal: 2 per CU (each holds 32 KB of stacks + the scene image) */
    uint32_t sky_blocks = 4096;          /* grid of the strided sky stage */
    bool sky_strided = false;            /* sky stage variant in use: fixed grid + grid stride (few misses) or one thread per entry */
    int sky_strided_mode = -1;           /* -1 automatic, 0 / 1 forced by RPT_SKY_STRIDED */

    /* scene */
    bool has_scene = false;
    DevBuf<float4> nodes, tri_geom, tri_shade, tri_tangent, mat_lite, per_vertex, materials, lds_image, light_rec;
    DevBuf<uint4> indices;
    DevBuf<float> tri_isect;
    DevBuf<float4> gpairs;                     /* pair records + links of the streamed global-memory walks (k_walk.h SceneViewPairsT) */
    DevBuf<uint32_t> glinks;
    DevBuf<float4> lds_image_shadow, gpairs_shadow;   /* the same tree with its pairs flipped for the fixed-order any-hit walks (shadow_order.h) */
    DevBuf<uint32_t> glinks_shadow;
    ShadowOrder shadow_order;
    DevBuf<float4> lds_image_last;                    /* pair records of the copy flipped for the hit-or-miss lanes of the last extension rays (choose_last_order) */
    LastOrder last_order;
    DevBuf<rpt_light_pick_entry> light_pick;
    DevBuf<uchar4> atlas;
    DevBuf<float4> skybox;
    DevScene scene{};
    uint32_t n_materials = 0;                  /* of the uploaded scene: what rpt_set_material_models' count must equal */
    /* rpt_set_material_models (rpt_models.hip): one record per material beside the material buffer — handed to k_shade_models as an argument of its own, DevScene
     * is what it was — and their host copy for rpt_material_models; both empty until set and after rpt_upload_scene */
    DevBuf<rpt_material_model> material_models;
    std::vector<rpt_material_model> material_models_host;
    bool models_in_use = false;                /* some record is not PBR: the shade stage is k_shade_models */
    bool force_model_kernels = false;          /* rpt_debug_force_model_kernels: k_shade_models whatever the records say (none: every material PBR) */
    /* rpt_set_material_volumes (rpt_volumes.hip): one absorption record per material, handed to k_shade_volumes as one more argument of its own, and their
     * host copy for rpt_material_volumes; the life cycle of the model records.  volumes_in_use is recomputed by both setters and both clears
     * (rpt_material_volumes_recount): it does not depend on the order in which the two record sets arrive */
    DevBuf<rpt_material_volume> material_volumes;
    std::vector<rpt_material_volume> material_volumes_host;
    bool volumes_in_use = false;               /* some Glass record has a volume record with a non-zero sigma: the shade stage is k_shade_volumes */
    bool force_volume_kernels = false;         /* rpt_debug_force_volume_kernels: k_shade_volumes whatever the records say */
    uint32_t last_shade_variant = 0;           /* rpt_debug_last_shade_variant: 0 k_shade, 1 k_shade_models, 2 k_shade_volumes, 3 k_shade_punctual — what the last shade launch was */
    /* rpt_set_punctual_lights (rpt_punctual.hip): four float4 per light (k_punctual.h), handed to k_shade_punctual as one more argument of its own, their host
     * records for rpt_punctual_lights, and the effective share of the first light draw: 0 with no lights, 1 over a scene without emissive triangles, else as set */
    DevBuf<float4> punctual_lights;
    std::vector<rpt_punctual_light> punctual_lights_host;
    float punctual_share = 0.0f;
    bool force_punctual_kernels = false;       /* rpt_debug_force_punctual_kernels: k_shade_punctual under NEE whatever the lights say (none: the parent's arithmetic) */
    /* rpt_set_camera_lens (rpt_lens.hip, k_lens.h): handed to the lens kernels as an argument of its own — DevConfig is what it was.  Active (anything but
     * {1, 0, *}): render calls open with k_generate_lens, complete with the lens builds of the completion kernels and keep at least two slots per pixel busy */
    rpt_camera_lens lens{1.0f, 0.0f, 1.0f, 0u};
    uint32_t bvh_depth = 0;
    int stack_cap = 16;

    /* config + partition */
    bool has_config = false;
    DevConfig cfg{};
    uint32_t n_slots = 0;       /* n_pixels << group_shift */
    uint32_t n_pixels = 0;      /* pixels of this rank's tiles */
    uint32_t group_shift = 0;   /* log2 of the samples of one pixel kept in flight (of the current / last rpt_render call) */
    uint32_t max_group_shift = 0, max_slots = 0;   /* what the state arrays are sized for */
    uint32_t sky_wide_cfg = 32768;       /* up to this many queued misses the sky march runs 16 lanes per miss */
    bool test_short_batch = false;       /* rpt_debug_short_batch: enqueue one iteration too few in an asynchronous batch (proves that the completion checks notice) */
    int samples_in_flight_request = 0;   /* 0 = automatic */
    uint32_t shadow_mode = RPT_SHADOW_EXACT;   /* rpt_set_shadow_mode: which any-hit walk rpt_launch_shadow enqueues (read at enqueue, nothing else depends on it) */
    uint64_t max_slots_budget = 160ull << 20;   /* automatic S: the most slots (pixels x samples in flight) a context allocates */
    std::vector<uint32_t> pixel_xy_host;
    DevBuf<uint32_t> pixel_xy;

    /* state */
    bool has_state = false;
    bool has_seeds = false;              /* rpt_reset has seeded the pixel state that is allocated now (the masked entry points insist on it) */
    DevBuf<float2> ray_b, hit;
    DevBuf<float4> ray_a, thr, rad, mis_a, mis_b, accum;
    DevBuf<uint2> rng;
    bool moments_on = false;             /* rpt_set_moments: render calls launch k_complete_moments and keep at least two slots per pixel busy (plan_slots) */
    DevBuf<float4> moments;              /* moments on: one record per owned pixel beside `accum`, same order (k_moments.h); zeroed whenever the accumulator is invalidated */
    DevBuf<unsigned long long> noise_counts;   /* rpt_noise_count: pixels, measured, above — allocated at its first use */
    DevBuf<uint32_t> q_sky, q_count;
    DevBuf<unsigned long long> ray_shards;
    DevBuf<float4> sh_o, sh_d, sh_c;
    DevBuf<DevStats> dev_stats;
    DevState state{};
    DevQueues queues{};
    uint32_t samples = 0;                /* the samples EVERY owned pixel received through uniform calls (what rpt_read_accum reports) */
    uint64_t accum_epoch = 0;            /* counts what invalidates the accumulator (rpt_reset, a resize): rpt_denoise_temporal promotes its history once per epoch */
    bool counts_nonuniform = false;      /* a masked pass gave samples to some owned pixels only: accum.w differs between pixels, the read-outs divide by it
                                            (k_adaptive.h mean_own).  Cleared by rpt_reset and by whatever invalidates the accumulator. */
    const PixelView *view = nullptr;     /* set for the duration of a masked pass's render call */
    AdaptiveState ad;
    bool first_walk_starts = false;   /* the current / last render call was opened without a pass over the slots: its first walk starts the paths (rpt_first_walk_starts_paths) */
    uint32_t call_samples = 0;  /* n_samples of the current / last rpt_render call (the shade stage of its first iteration derives what a slot owes) */

    /* scheduling: the traversal kernel reports each iteration's queue size into mapped pinned memory */
    PinnedBuf<unsigned long long> host_ring;       /* host view, RING entries */
    unsigned long long *host_ring_dev = nullptr;   /* device view of the same memory */

    /* stats */
    rpt_stats stats{};
    StageTimer timing;              /* RPT_STAGE_TIMING (rpt_destroy empties it before the stream goes) */
    bool async_pending = false;

    /* read-back and multi-GPU gather (rpt_comm.hip) */
    rpt_comm *comm = nullptr;
    DevBuf<float4> image;                 /* row-major W x H accumulator image (device), built by k_scatter_pixels (k_image_order.h) */
    PinnedBuf<float> host_image;          /* pinned twin of it: rpt_read_accum is one DMA */
    DevBuf<uint32_t> untile_map;          /* rpt_untile: destination map, rebuilt only when (W, H, world, stride) changes */
    uint64_t untile_key = 0;
    uint32_t untile_n = 0;

    DenoiseState dn;                      /* rpt_denoise.hip */
};

/* rpt_traverse.hip: the traversal stages (which walk kernel for the context's scene, on which grid) */
/* rpt_launch_nearest returns true when the launch it made also ENDED the paths it walked, so that no shade launch follows it in that iteration: the LAST
 * walk of an LDS-resident scene with several slots per pixel (emission added, HIT_DONE / sky queue written by the walk itself).
 * start_paths: iteration 0 of a call whose slots k_generate_first did not prepare (rpt_first_walk_starts_paths: the FIRST walk computes each slot's
 * camera ray where it takes the slot; render_impl then opens the call with a one-workgroup k_generate_first that only zeroes the counters). */
bool rpt_launch_nearest(rpt_ctx *c, uint32_t iteration, bool last_without_nee /* the last extension rays of a batch of known length, no NEE */,
                        bool camera_rays /* iteration 0 of a render call: every ray leaves cfg.cam_position */, bool start_paths);
bool rpt_first_walk_starts_paths(const rpt_ctx *c);
void rpt_launch_shadow(rpt_ctx *c);
/* rpt_models.hip: the shade stage of one iteration as k_shade_models (NEE mode, textured or not, packed or not as launch_iteration picks k_shade), and
 * "no records", for rpt_upload_scene */
void rpt_launch_shade_models(rpt_ctx *c, uint32_t iteration, uint32_t blocks);
void rpt_material_models_clear(rpt_ctx *c);
/* rpt_volumes.hip: the same stage as k_shade_volumes; "no volume records", for rpt_upload_scene; volumes_in_use from the two record sets as they stand */
void rpt_launch_shade_volumes(rpt_ctx *c, uint32_t iteration, uint32_t blocks);
void rpt_material_volumes_clear(rpt_ctx *c);
void rpt_material_volumes_recount(rpt_ctx *c);
/* rpt_punctual.hip: the same stage as k_shade_punctual (NEE modes 1 and 2 only); "no lights", for rpt_upload_scene */
void rpt_launch_shade_punctual(rpt_ctx *c, uint32_t iteration, uint32_t blocks);
void rpt_punctual_lights_clear(rpt_ctx *c);
/* what rpt_set_punctual_lights refuses without looking at a context (the message as the setter gives it), and the device records of k_punctual.h */
int rpt_punctual_lights_check(const rpt_punctual_light *lights, size_t n, float pick_share, bool mesh_lights, std::string &error);
std::vector<float4> rpt_punctual_records(const rpt_punctual_light *lights, size_t n);
/* rpt_lens.hip: the lens is anything but the reference's camera; its primary rays leave different origins (aperture > 0: iteration 0 is the plain walk) */
inline bool rpt_lens_active(const rpt_ctx *c) { return !(c->lens.tan_half_fov == 1.0f && c->lens.aperture_radius == 0.0f); }
inline bool rpt_lens_scatters_origins(const rpt_ctx *c) { return c->lens.aperture_radius > 0.0f; }
/* the opening pass of a render call under an active lens (k_generate_lens over all slots, in place of k_generate_first), its completion kernel (in place of
 * k_complete / k_complete_moments, same grid and LDS) and the centre rays of the denoiser's guides (in place of k_dn_camera_rays) */
void rpt_launch_generate_lens(rpt_ctx *c, uint32_t n_samples, uint32_t blocks);
void rpt_launch_complete_lens(rpt_ctx *c, uint32_t iteration, uint32_t final_pass, uint32_t waves, size_t lds_bytes);
void rpt_launch_guide_rays_lens(rpt_ctx *c, const uint32_t *order, uint32_t n, float *origins, float *dirs);
/* rpt_hip.hip: the LDS dimensions a configuration's paths draw (kernels/src/rng.rs:20-21,51-54; the table has 31 usable), and the refusal of an aperture
 * under a configuration that needs all 31 — entry 31 is the lens sample's (k_lens.h); `who`: the entry point that came second */
uint64_t rpt_config_dimensions(const rpt_tracing_config &cfg);
int rpt_lens_check_dimensions(rpt_ctx *c, const rpt_tracing_config &cfg, const rpt_camera_lens &lens, const char *who);
void rpt_launch_trace_debug(rpt_ctx *c, int any_hit /* 0 nearest, 1 any-hit, 2 segment-bounded any-hit */, uint32_t n, const float *origins, const float *dirs, const float *max_t, float *out_t, uint32_t *out_tri,
                            uint32_t *out_flags);
hipError_t rpt_last_walk_attributes(hipFuncAttributes *out);      /* of k_traverse_nearest_stream<.., LAST>: its static LDS decides whether the flipped copy fits */
/* rpt_hip.hip, for the production-trace hook of rpt_debug.hip: the per-slot arrays for a call over `n` slots (grown, never shrunk), and "nothing in
 * flight" on the context's stream — queue counters zeroed, every slot of the current call idle (k_fill_idle is compiled in rpt_hip.hip only) */
int ensure_slot_state(rpt_ctx *c, size_t n, bool need_shadow, bool need_mis);
int rpt_idle_all_slots(rpt_ctx *c);
/* rank-local slot order (rpt_hip.hip) */
void rpt_build_pixel_order(uint32_t W, uint32_t H, uint32_t rank, uint32_t world, std::vector<uint32_t> &out);
/* the rank's tiles in that order, four words each — first entry of the order, pixel count, x | y << 16 of the origin, 0 (k_adaptive.h AdTile) */
void rpt_build_tile_table(uint32_t W, uint32_t H, uint32_t rank, uint32_t world, std::vector<uint32_t> &out);
/* rpt_comm.hip: called by rpt_hip.hip when the context goes away */
void rpt_comm_release(rpt_ctx *c);
/* rpt_comm.hip, for rpt_denoise(RPT_DENOISE_GATHERED): the image of the last gather on rank 0 of a communicator, once that gather has completed, its sample
 * count, whether the counts were non-uniform when it was snapshotted, and the stream the gather ran on (work on it is ordered after the gather and overlaps the batch on the context's own stream) */
int rpt_comm_gathered_image(rpt_ctx *c, const float4 **image_out, uint32_t *samples_out, bool *nonuniform_out, hipStream_t *stream_out);
/* rpt_comm.hip: rpt_gather_set_moments is on (rpt_set_moments refuses to turn the record off then; the denoisers take the gathered record for a null image) */
bool rpt_comm_gather_moments_on(const rpt_ctx *c);
/* rpt_comm.hip, for rpt_denoise_variance / rpt_denoise_temporal (RPT_DENOISE_GATHERED, no caller's image, the setting on): the row-major moments image of
 * the last gather on rank 0 — written on the stream rpt_comm_gathered_image hands out; RPT_EINVAL (named after `who`) until a gather has carried moments */
int rpt_comm_gathered_moments(rpt_ctx *c, const char *who, const float4 **moments_out);
/* rpt_moments.hip: the moments record of a context with moments on, for its current pixel count: allocated if need be and zeroed on the context's stream */
int rpt_moments_reset(rpt_ctx *c);
/* rpt_moments.hip, for rpt_multi_render_to_noise (rpt_comm.hip): the loop of rpt_render_to_noise over the caller's "render n more samples" and "count" */
int rpt_render_to_noise_with(const rpt_noise_target *target, rpt_noise_result *out, std::string &error, int (*render)(void *, uint32_t), int (*count)(void *, float, rpt_noise_counts *),
                             void *who);
/* rpt_hip.hip, for rpt_adaptive.hip: n_samples more samples for the pixels of `view` through the pipeline of rpt_render_async (returns once enqueued when the
 * batch's length is known).  Counts view->n_pixels x n_samples into rpt_stats.samples and nothing into the context's uniform sample count. */
int rpt_render_view(rpt_ctx *c, uint32_t n_samples, const PixelView *view);
/* rpt_adaptive.hip, for the rpt_multi_* forms (rpt_comm.hip): the three steps of a masked pass on one rank, so that several ranks' passes overlap.
 * select: flags, counts and scan enqueued on the context's stream (mask != null: the byte mask; else the selection rule on the moments with `target` —
 * radius 0: a pixel's own noise, the kernels of rpt_render_adaptive; 1 .. RPT_ADAPTIVE_MAX_RADIUS: the window rule, k_ad_window);
 * selected: waits and reads what was selected; pass: gather what was last read as selected, n_samples through rpt_render_view, scatter back (nothing when nothing was). */
struct rpt_adaptive_selection { uint32_t n_active, z_min, z_max; rpt_noise_counts counts; };
int rpt_adaptive_select(rpt_ctx *c, const uint8_t *mask, const rpt_noise_target *target, uint32_t radius);
int rpt_adaptive_selected(rpt_ctx *c, bool with_counts, rpt_adaptive_selection *out);
int rpt_adaptive_pass(rpt_ctx *c, uint32_t n_samples, bool uniform_ok /* a pass that selected every owned pixel may run as the uniform call it is */);
/* rpt_moments.hip: the refusals of a noise target, named after the entry point `who` */
int rpt_noise_check_target(const rpt_noise_target &t, std::string &error, const char *who);
/* the loop of rpt_render_adaptive / rpt_multi_render_adaptive over the caller's "n uniform samples", "select and report" and "render the selected" */
struct rpt_adaptive_driver {
    int (*render)(void *who, uint32_t n_samples, uint64_t *pixel_samples_out);
    int (*select)(void *who, const rpt_noise_target *target, rpt_adaptive_selection *out);
    int (*pass)(void *who, uint32_t n_samples);
};
/* rpt_adaptive.hip, for rpt_multi_adaptive_mask: what rpt_adaptive_mask refuses, named after `who`; and the call itself after the checks */
int rpt_adaptive_mask_check(rpt_ctx *c, const rpt_noise_target *target, uint32_t radius, std::string &error, const char *who);
/* rpt_resolve while the counts are non-uniform: every pixel's sum by its own accum.w (its kernel is compiled in rpt_adaptive.hip, so that the code object of
 * rpt_hip.hip — the pipeline's kernels — is the one it was) */
int rpt_resolve_own(rpt_ctx *c, uint32_t tonemap_op, float *out_rgb);
int rpt_render_adaptive_with(const rpt_noise_target *target, rpt_adaptive_result *out, const rpt_adaptive_driver &driver, void *who);
/* rpt_denoise.hip: the denoiser's buffers go (a resize), or buffers and events (the context goes away: while its device is current) */
void rpt_denoise_release(rpt_ctx *c, bool events_too);
/* rpt_hip.hip: DevConfig::euler of a configuration's cam_rotation */
void rpt_camera_matrix(const float *cam_rotation, float *euler_out);
std::string &rpt_create_error();

/* RPT_UPLOAD_TIMING=1: host-side section times of rpt_upload_scene / rpt_bvh_build_gpu on stderr (where the start-up time of a large scene goes) */
struct SectionTimer {
    bool on;
    const char *title;
    std::chrono::steady_clock::time_point last;
    std::string line;
    explicit SectionTimer(const char *t) : on(rpt_read_knobs().upload_timing), title(t), last(std::chrono::steady_clock::now()) {}
    void mark(const char *name) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        char buf[96];
        snprintf(buf, sizeof buf, " %s %.1f", name, std::chrono::duration<double, std::milli>(now - last).count());
        line += buf;
        last = now;
    }
    ~SectionTimer() { if (on) fprintf(stderr, "%s (ms):%s\n", title, line.c_str()); }
};

#endif /* RPT_CTX_H */
