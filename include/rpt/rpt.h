/*
 * rpt.h — C ABI of librpt_hip.so, the MI355X (gfx950) wavefront path tracer
 * that drops in behind the reference's render dispatch.
 *
 * Boundary being replaced: `trace_gpu` in the reference, src/trace.rs:136-224,
 * which today drives one SPIR-V megakernel through gpgpu-rs/wgpu.  Each entry
 * point below cites the reference call(s) it stands in for.  All functions are
 * `extern "C"`, take plain pointers and sizes in the `shared_structs` layouts
 * (include/rpt/shared_structs.h), never throw, never abort, never call exit():
 * return 0 on success or a negative RPT_E* code, with a message available from
 * rpt_last_error().
 *
 * Ownership: the caller owns every host pointer passed in; the library copies
 * during the call.  Device memory belongs to the rpt_ctx and is released by
 * rpt_destroy().  A context is single-caller (the reference uses one render
 * thread, src/app.rs:157-164); distinct contexts may live on distinct threads.
 */
#ifndef RPT_H
#define RPT_H

#include <stddef.h>
#include <stdint.h>
#include "shared_structs.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RPT_ABI_VERSION 3

enum {
    RPT_OK = 0,
    RPT_EINVAL = -1,     /* bad argument / call order                             */
    RPT_ENODEV = -2,     /* no usable HIP device                                   */
    RPT_EHIP = -3,       /* a HIP runtime call failed (message has the HIP text)   */
    RPT_ECONFIG = -4,    /* config the reference itself would panic on (see below) */
    RPT_ESCENE = -5,     /* scene buffers inconsistent (index out of range, BVH too deep) */
    RPT_ENOMEM = -6
};

typedef struct rpt_ctx rpt_ctx;

/* Counters of one context since the last rpt_reset().  Ray counting rule
 * (SURVEY.md §8d): one extension ray per executed intersect_nearest
 * (kernels/src/lib.rs:63), one shadow ray per executed intersect_any
 * (kernels/src/light_pick.rs:141). */
typedef struct rpt_stats {
    uint64_t samples;          /* pixel-samples accumulated (W*H*spp on a full image)   */
    uint64_t extension_rays;
    uint64_t shadow_rays;
    uint64_t sky_evals;        /* misses shaded by the procedural / image sky             */
    uint64_t light_index_clamped; /* gen_r1()==1.0 alias-table overruns clamped (Appendix C) */
    uint64_t iterations;       /* wavefront iterations executed                           */
    double   render_ms;        /* wall time of rpt_render calls, host clock               */
    double   kernel_ms[8];     /* HIP-event time per stage: see RPT_STAGE_*               */
    uint64_t kernel_launches[8];
    uint64_t shadow_rays_elided; /* of shadow_rays: NEE evaluations whose shadow ray was not walked because the term it gates is zero
                                    whatever the walk finds (light_pdf = 0 or bsdf_pdf = 0, light_pick.rs:150-158); rays traced on the
                                    device = extension_rays + shadow_rays - shadow_rays_elided */
} rpt_stats;

enum {
    RPT_STAGE_GENERATE = 0,    /* camera rays + accumulate/regenerate */
    RPT_STAGE_TRAVERSE = 1,    /* nearest-hit BVH traversal           */
    RPT_STAGE_SHADE = 2,       /* material, BSDF sample, NEE setup    */
    RPT_STAGE_SHADOW = 3,      /* any-hit traversal + NEE resolve     */
    RPT_STAGE_SKY = 4,         /* miss shading                        */
    RPT_STAGE_COMPLETE = 5,    /* a batch's one completion pass: radiances of a generation added to the accumulator in sample order */
    RPT_STAGE_COUNT = 6
};

/* Replaces the lazy wgpu framework/adaptor creation, src/trace.rs:3-6,25-38.
 * device_id is a HIP ordinal. */
int rpt_create(int device_id, rpt_ctx **out);

/* Multi-GPU tile partition (no reference equivalent: the reference is single
 * device).  The W x H framebuffer is cut into RPT_TILE x RPT_TILE pixel tiles;
 * tile t belongs to rank (t mod world_size).  Must be called before
 * rpt_set_config; default is rank 0 of 1 (whole image). */
#define RPT_TILE 64
int rpt_set_partition(rpt_ctx *ctx, uint32_t rank, uint32_t world_size);

/* Tuning knob without reference equivalent: how many samples of one pixel are kept
 * in flight (rounded up to a power of two, <= 32).  0 = automatic (enough to give
 * the GPU ~0.75 M concurrent paths when this rank owns few pixels).  The result
 * does not depend on it: finished samples are added to a pixel's accumulator in
 * sample order whatever the value.  Invalidates the accumulator like a resize:
 * call before rpt_set_config or re-run rpt_reset afterwards. */
int rpt_set_samples_in_flight(rpt_ctx *ctx, int samples);

/* Replaces World::into_gpu (src/asset.rs:226-235), BVH::into_gpu
 * (src/bvh.rs:40-43) and the skybox upload (src/trace.rs:144).  Buffers are in
 * the order the reference binds them (kernels/src/lib.rs:195-202).  atlas and
 * skybox may be NULL (no textures / procedural sky).  atlas is RGBA8 as in
 * asset.rs:231 and is sampled with the CPU polyfill's semantics
 * (shared_structs/src/image_polyfill.rs:38-55; texel = u8/255, alpha = 1,
 * src/asset.rs:266-273).  skybox is float RGBA, same sampler. */
int rpt_upload_scene(rpt_ctx *ctx,
                     const rpt_per_vertex_data *per_vertex, size_t n_vertices,
                     const rpt_triangle *indices, size_t n_triangles,
                     const rpt_bvh_node *nodes, size_t n_nodes,
                     const rpt_material_data *materials, size_t n_materials,
                     const rpt_light_pick_entry *light_pick, size_t n_light_pick,
                     const uint8_t *atlas_rgba8, uint32_t atlas_w, uint32_t atlas_h,
                     const float *skybox_rgba32f, uint32_t sky_w, uint32_t sky_h);

/* Replaces GpuUniformBuffer::from_slice / config_buffer.write
 * (src/trace.rs:168,219).  Rejects with RPT_ECONFIG what the reference's CPU
 * path would panic on: more LDS dimensions than the 32-entry table
 * (kernels/src/rng.rs:20-21), i.e. 2 + max_bounces*(3 + 4*[nee!=0]) +
 * max(0, max_bounces-1-min_bounces) > 31. Changing width/height invalidates
 * the accumulator: call rpt_reset afterwards. */
int rpt_set_config(rpt_ctx *ctx, const rpt_tracing_config *config);

/* Replaces rng_buffer / output_buffer creation and the flush path
 * (src/trace.rs:164-170, 219-221).  rng_seed has width*height entries, pixel
 * index y*width + x; accum_init_rgba (nullable) is width*height float4 =
 * mean * samples for resume (src/trace.rs:163-164), with samples_init the
 * matching sample count. */
int rpt_reset(rpt_ctx *ctx, const rpt_rng_state *rng_seed,
              const float *accum_init_rgba, uint32_t samples_init);

/* Replaces the `for _ in 0..sync_rate { enqueue; poll_blocking }` loop
 * (src/trace.rs:182-194) — one call renders n_samples more samples for every
 * pixel of this rank's tiles with no per-sample host round trip.  Per pixel the
 * effect is exactly n_samples times `output[i] += (radiance, 1); rng[i].x += 1`
 * (kernels/src/lib.rs:225-226) in sample order. Synchronous on return. */
int rpt_render(rpt_ctx *ctx, uint32_t n_samples);

/* rpt_render that returns as soon as the batch is enqueued — possible when its iteration count is known up front,
 * i.e. when no slot gets a second sample in this call (n_samples <= slots per pixel, the usual batch); otherwise it
 * behaves exactly like rpt_render.  Results are read through the same entry points (each synchronises by itself).
 * rpt_wait blocks until everything enqueued so far has completed.  rpt_stream hands out the HIP stream
 * (hipStream_t) the library works on, so that a caller can order its own copies / collectives after a batch without
 * a host round trip (bench.py wraps it as a torch ExternalStream for the per-batch gather). */
int rpt_render_async(rpt_ctx *ctx, uint32_t n_samples);
int rpt_wait(rpt_ctx *ctx);
int rpt_stream(rpt_ctx *ctx, void **hip_stream_out);

/* Replaces output_buffer.read_blocking (src/trace.rs:198).  Writes the SUM
 * (not the mean) as width*height float4 (r, g, b, sample count) in row-major,
 * y-down order.  Pixels of tiles owned by other ranks are written as zeros.
 * The tile-major block is un-tiled on the device and leaves it as one DMA into
 * pinned memory owned by the context; rpt_map_accum hands out that buffer itself
 * (valid until the next rpt_read_accum / rpt_map_accum / rpt_set_config on the
 * context), rpt_read_accum copies it into the caller's. */
int rpt_read_accum(rpt_ctx *ctx, float *out_rgba, uint32_t *out_samples);
int rpt_map_accum(rpt_ctx *ctx, const float **out_rgba, uint32_t *out_samples);

/* Post-accumulation step on the device: mean = sum / samples
 * (src/trace.rs:199-204) then tonemap operator 0..6 exactly as the display shader
 * numbers them (src/resources/render.wgsl:131-153: 0 none, 1 Reinhard, 2 ACES
 * Narkowicz x0.6, 3 ACES Narkowicz, 4 ACES Hill, 5 Neutral, 6 Uncharted).  Writes
 * width*height*3 floats, row-major; other ranks' pixels are zero. */
int rpt_resolve(rpt_ctx *ctx, uint32_t tonemap_op, float *out_rgb);

/* Reads back rng[i] (n, offset) for every pixel (other ranks' pixels: zeros);
 * lets a caller verify `rng[i].x += 1` semantics (kernels/src/lib.rs:226). */
int rpt_read_rng(rpt_ctx *ctx, rpt_rng_state *out);

/* --- multi-GPU gather support ---------------------------- */
/* This rank's accumulators live in ONE contiguous tile-major device block of
 * rpt_local_pixels() float4: tiles in ascending tile id; inside a tile 8x8
 * pixel blocks row-major, pixels row-major inside a block; pixels outside the
 * image skipped (rpt_tile_order gives the exact order).  The caller (one
 * process per GPU) hands that pointer to its RCCL gather and gives the root
 * the concatenation. */
/* Pure function, no context / GPU needed: writes the (x | y << 16) pixel
 * coordinates of rank's block, in block order, into out_xy (capacity entries)
 * and the count into *n. out_xy may be NULL to query the count. */
int rpt_tile_order(uint32_t width, uint32_t height, uint32_t rank, uint32_t world_size,
                   uint32_t *out_xy, size_t capacity, size_t *n);
int rpt_local_pixels(rpt_ctx *ctx, uint64_t *n_pixels);
/* No synchronisation: order your work after the batch on rpt_stream().  The pointer is invalidated by
 * rpt_set_config (resize), rpt_set_partition and rpt_set_samples_in_flight. */
int rpt_local_block_device_ptr(rpt_ctx *ctx, void **dev_ptr);
/* Pixel count of any rank's block for the current config (for gather sizes). */
int rpt_rank_pixels(rpt_ctx *ctx, uint32_t rank, uint64_t *n_pixels);
/* For callers that run their own collective: scatter the `world_size` gathered tile-major blocks (device memory)
 * into a row-major width*height float4 image in device memory, on the context's stream — launch only (the destination
 * map is rebuilt when the configuration changes, never per batch); synchronise with rpt_wait.  Block r starts at
 * element r * block_stride_pixels (a gather into equal-sized padded slots), or the blocks are tightly concatenated
 * when block_stride_pixels == 0. */
int rpt_untile(rpt_ctx *ctx, const void *dev_gathered_blocks, uint64_t block_stride_pixels, void *dev_out_image);

/* The gather itself, inside the library: RCCL (ncclSend / ncclRecv, grouped) over xGMI, on a second HIP stream.
 *   one process per GPU:  rank 0 calls rpt_comm_unique_id and hands the 128 bytes to every rank by any means (file,
 *                         socket, torch.distributed); every rank calls rpt_comm_init (= ncclCommInitRank on the
 *                         context's device + rpt_set_partition(rank, world_size)).
 *   after a batch:        rpt_gather_async — stream-ordered after everything enqueued so far (rpt_render_async
 *                         included): the accumulators are snapshotted, the blocks travel to rank 0 and are un-tiled
 *                         there while the next batch renders.  Collective: every rank must call it, in the same order.
 *                         Nothing is allocated, copied from the host or synchronised per call.
 *   rank 0:               rpt_read_gathered (host, W*H float4, the whole image) or rpt_gathered_device_ptr;
 *                         rpt_gather_wait blocks until the last gather has completed. */
#define RPT_COMM_ID_BYTES 128
int rpt_comm_unique_id(uint8_t *id_out /* RPT_COMM_ID_BYTES */);
int rpt_comm_init(rpt_ctx *ctx, const uint8_t *unique_id, uint32_t rank, uint32_t world_size);
/* One GPU, no RCCL: the same snapshot / second stream / un-tile / pinned DMA for a single context, so that the reference's
 * loop (render a batch, read it back: src/trace.rs:182-204) reads batch k while batch k+1 renders:
 *   rpt_render_async ; rpt_gather_async ; rpt_render_async (next batch) ; rpt_read_gathered -> the image after the first. */
int rpt_comm_init_local(rpt_ctx *ctx);
int rpt_comm_world(rpt_ctx *ctx, uint32_t *rank_out, uint32_t *world_size_out);   /* as RCCL reports it (ncclCommCount) */
/* Which collective library the process resolved (dlopen): "librccl.so.1" ..., "" before the first communicator, or the path
 * given in RPT_RCCL_LIBRARY — an override that exists for tests/fake_rccl (N processes on a one-GPU test box); a
 * measurement made with it set is not a measurement of RCCL, and bench.py refuses to run then. */
const char *rpt_comm_library(void);
int rpt_gather_async(rpt_ctx *ctx);
int rpt_gather_wait(rpt_ctx *ctx);
int rpt_read_gathered(rpt_ctx *ctx, float *out_rgba, uint32_t *out_samples);
int rpt_gathered_device_ptr(rpt_ctx *ctx, void **dev_ptr);

/* --- the moments record and the counts flag inside the gather -------------------------------------------------------------------------------------
 * Opt-in, a second wire format of the same gather: with the setting off (the default) the gather, its bytes and its kernels are what they were.
 * With it on, a rank's message is its whole slot — [accumulator block][moments record][trailer of four words: a format word, the rank's
 * counts_nonuniform, its uniform sample count, its pixel count] — in the one ncclSend / ncclRecv per peer of the one group; rank 0 un-tiles both records
 * (a second row-major width*height float4 image beside the gathered one) and folds the trailers into rpt_gathered_info, all on the gather's stream.
 * Nothing is allocated, copied from the host or synchronised per gather; batch k + 1 renders while accumulators AND moments of batch k travel.
 *
 * rpt_gather_set_moments(ctx, 1)   needs a communicator (rpt_comm_init, rpt_comm_init_local, a context of an rpt_multi), else RPT_EINVAL.  Turns the
 *                  context's moments on if they are off and leaves them on (as rpt_render_to_noise does), synchronises both streams and re-sizes the
 *                  gather buffers (zeroed: no uninitialised memory travels).  No gathered image exists afterwards until the next gather, as after a
 *                  resize.  While it is on, rpt_set_moments(ctx, 0) is refused with RPT_EINVAL (rpt_gather_set_moments(ctx, 0) is the way out): a
 *                  rank's message length stays a function of (width, height, world, setting) alone.
 *                  COLLECTIVE, like the configuration and like rpt_gather_async ("every rank must call it, in the same order"): every rank of a
 *                  communicator must hold the same value at every gather.  rpt_multi_gather_set_moments sets every rank in one call.
 *                  (ctx, 0) restores the plain format and every refusal of the plain format, word for word.
 * With the setting on, on rank 0:
 *   rpt_denoise_variance / rpt_denoise_temporal (RPT_DENOISE_GATHERED, moments_xyzw == NULL) filter by the gathered record, from device memory, on the
 *                  gather's stream: no host trip.  RPT_EINVAL until a gather has carried moments; a caller's image still takes precedence when given.
 *   rpt_denoise, rpt_denoise_variance, rpt_denoise_temporal (RPT_DENOISE_GATHERED) divide every pixel by its own .w iff rpt_gathered_info.nonuniform:
 *                  the decision comes from every rank's trailer, no longer from rank 0's own flag (ranks of a process-per-GPU run are masked
 *                  differently as a rule: rpt_render_adaptive on each).
 *   rpt_read_gathered_moments   width*height float4, row-major: what rpt_read_moments of one context that rendered everything returns.
 *   rpt_gathered_moments_device_ptr   the device image itself, as rpt_gathered_device_ptr (no synchronisation: rpt_gather_wait first).
 *   rpt_read_gathered's out_samples stays rank 0's own count; rpt_gathered_info_get is where a caller sees disagreement.
 * rpt_gathered_info_get (rank 0, after a gather; waits for it): with_moments = the last gather carried the records.  Then nonuniform = the OR over the
 *                  ranks that own pixels of counts_nonuniform at their snapshot, or samples_min != samples_max; samples_min / samples_max of those ranks'
 *                  uniform sample counts at their snapshot; bad_trailers = ranks whose trailer did not carry the format word (0 unless the setting
 *                  differs between ranks: then the image is not to be trusted).  After a plain gather: with_moments = 0, nonuniform = the snapshot's
 *                  flag of this context (rpt_multi: of any rank), samples_min = samples_max = out_samples of rpt_read_gathered, bad_trailers = 0.
 * RPT_EINVAL for null pointers, from the read-outs on a rank other than 0, with the setting off, before a gather has carried moments and after a
 * resize until the next gather; the context stays usable. */
typedef struct rpt_gathered_info {
    uint32_t with_moments;
    uint32_t nonuniform;
    uint32_t samples_min, samples_max;
    uint32_t bad_trailers;
    uint32_t reserved[3];
} rpt_gathered_info;
int rpt_gather_set_moments(rpt_ctx *ctx, uint32_t on);     /* default 0 */
int rpt_gather_moments(rpt_ctx *ctx, uint32_t *on_out);
int rpt_read_gathered_moments(rpt_ctx *ctx, float *out_xyzw);
int rpt_gathered_moments_device_ptr(rpt_ctx *ctx, void **dev_ptr);
int rpt_gathered_info_get(rpt_ctx *ctx, rpt_gathered_info *out);

/* ONE process driving every GPU of the node — the shape the reference's single render thread (src/trace.rs:136-224,
 * src/app.rs:157-164) can call: the same entry points as above, fanned out over n_devices contexts created with
 * ncclCommInitAll; the caller sees one W x H image.  rpt_multi_render = one batch on every GPU + the batch's single
 * gather, returns once enqueued; rpt_multi_read_accum waits and returns the whole image from rank 0.
 * RPT_MULTI_ALLOW_SHARED_DEVICE: test aid for boxes with one GPU — a device may be listed several times; ranks then
 * exchange their blocks by stream-ordered device copies instead of RCCL (which refuses two ranks on one device). */
typedef struct rpt_multi rpt_multi;
#define RPT_MULTI_ALLOW_SHARED_DEVICE 1u
int rpt_multi_create(const int *device_ids, int n_devices, uint32_t flags, rpt_multi **out);
int rpt_multi_size(rpt_multi *m);
rpt_ctx *rpt_multi_ctx(rpt_multi *m, int rank);        /* e.g. for rpt_set_samples_in_flight / rpt_get_stats per GPU */
int rpt_multi_upload_scene(rpt_multi *m,
                           const rpt_per_vertex_data *per_vertex, size_t n_vertices,
                           const rpt_triangle *indices, size_t n_triangles,
                           const rpt_bvh_node *nodes, size_t n_nodes,
                           const rpt_material_data *materials, size_t n_materials,
                           const rpt_light_pick_entry *light_pick, size_t n_light_pick,
                           const uint8_t *atlas_rgba8, uint32_t atlas_w, uint32_t atlas_h,
                           const float *skybox_rgba32f, uint32_t sky_w, uint32_t sky_h);
int rpt_multi_set_config(rpt_multi *m, const rpt_tracing_config *config);
int rpt_multi_reset(rpt_multi *m, const rpt_rng_state *rng_seed, const float *accum_init_rgba, uint32_t samples_init);
int rpt_multi_set_shadow_mode(rpt_multi *m, uint32_t mode);  /* rpt_set_shadow_mode (below) on every rank */
/* (rpt_multi_set_material_models: with the material models, below) */
/* (rpt_multi_set_moments, rpt_multi_read_moments, rpt_multi_noise_count, rpt_multi_render_to_noise: with the moments, below) */
int rpt_multi_render(rpt_multi *m, uint32_t n_samples);
int rpt_multi_wait(rpt_multi *m);
int rpt_multi_read_accum(rpt_multi *m, float *out_rgba, uint32_t *out_samples);
int rpt_multi_get_stats(rpt_multi *m, rpt_stats *out);      /* counters summed, times = max over GPUs */
void rpt_multi_destroy(rpt_multi *m);
const char *rpt_multi_last_error(rpt_multi *m);

int rpt_get_stats(rpt_ctx *ctx, rpt_stats *out);
void rpt_destroy(rpt_ctx *ctx);
/* ctx may be NULL: returns the last error of a failed rpt_create on this thread. */
const char *rpt_last_error(rpt_ctx *ctx);
int rpt_abi_version(void);
/* tools/source_fingerprint.py of the device-side sources this library was built from ("unknown" for a build outside the Makefile):
 * profiles/traffic_*.json carry the same value, and bench.py reports counter-derived figures only when they match. */
const char *rpt_build_fingerprint(void);
/* compute units and peak engine clock of a HIP device, as the runtime reports them (bench.py: SIMD issue cycles available) */
int rpt_device_info(int device_id, uint32_t *compute_units_out, uint32_t *clock_khz_out);
/* Which visiting order the shadow (any-hit) walks of the uploaded scene use, and the probe that decided it.  The reference's shadow query
 * reads `.hit` only (kernels/src/light_pick.rs:148) and `.hit` does not depend on the order siblings are visited in (intersection.rs:191-213),
 * so the library may choose: fixed_out = 0 the reference's near-first order, 1 a fixed opaque-first order over a flipped copy of the tree —
 * chosen at rpt_upload_scene by the node visits of synthetic shadow rays under both (csrc/shadow_order.h).  The image is the same either way. */
int rpt_shadow_order(rpt_ctx *ctx, uint32_t *fixed_out, double *visits_near_out, double *visits_fixed_out, uint32_t *probe_rays_out, double *probe_ms_out);
/* Which any-hit walk the shadow rays of the batches enqueued from now on take.  Opt-in: the default, what bench.py measures and what every parity
 * statement of this header is about, is RPT_SHADOW_EXACT.
 *   RPT_SHADOW_EXACT    the reference's walk: boxes are pruned against result.t, which stays 1e6 until the first accept (intersection.rs:212-213), so an
 *                       unoccluded shadow ray enters every box on its line to the far wall.  `.hit` is the reference's, bit for bit.
 *   RPT_SHADOW_SEGMENT  a child box is entered iff the reference's test passes (tmax >= tmin && tmax > 0 && tmin < 1e6, intersection.rs:117) AND
 *                       tmin <= max_t, max_t being the ray's own bound, the distance to the light point (light_pick.rs:141).  Nothing else changes: the triangle
 *                       accept test (t > 0.001 && t < 1e6 && t <= max_t), the root (never box-tested), which rays are elided, the ray counts of rpt_stats.
 *                       For max_t >= 1e6 it is the exact walk.
 * Pruning only removes boxes, so a SEGMENT hit implies the reference's: an occlusion is never gained.  One can be lost, and the image differ from the
 * reference's, only through a triangle whose computed t <= max_t lies in a box whose computed tmin > max_t (box-t and triangle-t round differently).  On the
 * CPU model (tools/anyhit_order_sim.cpp sim_any_hit_segment) that happened for 0 of 10^6 adversarial rays over the four shipped scenes (tests/test_shadow_segment.py)
 * and for 0 of the 12.0 M shadow rays two samples per pixel of DarkCornell 1024^2 and VeachMIS 1080p trace; the same model prices the walk at 40-50 % fewer
 * wave-instructions per shadow ray (profiles/r10_anyhit_sim_segment.txt).
 * Measured on one MI355X at 32 samples per pixel (tools/shadow_mode_ab.py, profiles/r10_shadow_segment_ab.txt; bench.py's figures are the EXACT mode's):
 *   DarkCornell 1024^2 MIS   batch 20.5 -> 18.5 ms (-10 %), shadow stage 5.99 -> 3.76 ms    0 accumulator words differ (115 M shadow rays)
 *   VeachMIS 1080p MIS       batch 28.9 -> 24.8 ms (-14 %), shadow stage 9.01 -> 4.56 ms    30 words = 10 of 2.07 M pixels differ (77 M shadow rays)
 *   1 M-triangle stand-in    batch 324.7 -> 318.6 ms (-2 %), shadow stage 118.7 -> 112.6    12 words = 4 of 4.2 M pixels differ (397 M shadow rays)
 * A pixel that differs lost one occlusion in 32 samples: it is brighter by one NEE term — VeachMIS's ten by 0.005 - 0.3 % of their value, more than the per-pixel
 * 1e-4 of BASELINE.md's contract at those pixels; every other pixel is the EXACT image bit for bit, and each of the ten is a pixel where the CPU model of the rule
 * loses the same occlusion (tests/test_gpu_shadow_segment.py, profiles/r10_shadow_segment_parity.txt; the stand-in's four were counted, not traced back).  So: inside the contract except at a handful of pixels per million,
 * outside the bit-for-bit one.
 * Callable at any time between batches: nothing is reallocated, the accumulator stays valid, batches already enqueued keep the mode they were enqueued
 * with.  Any other value: RPT_EINVAL, the mode stays.  There is no environment variable for it: those (rpt_knobs) never change a result. */
enum { RPT_SHADOW_EXACT = 0, RPT_SHADOW_SEGMENT = 1 };
int rpt_set_shadow_mode(rpt_ctx *ctx, uint32_t mode);
int rpt_shadow_mode(rpt_ctx *ctx, uint32_t *mode_out);
/* Material models.  Opt-in; no reference equivalent as a call: the reference's kernels crate carries Lambertian (kernels/src/bsdf.rs:46-105) and Glass
 * (bsdf.rs:107-176) behind its BSDF trait and constructs neither (lib.rs:144 always calls get_pbr_bsdf).  A material's model replaces the BSDF constructed at
 * lib.rs:144 and nothing else of lib.rs:21-186.  With pbr = get_pbr_bsdf(config, material, uv, atlas) exactly as without models (texture lookups and its two
 * guards included):
 *   RPT_MODEL_PBR         pbr
 *   RPT_MODEL_LAMBERTIAN  Lambertian { albedo: pbr.albedo }
 *   RPT_MODEL_GLASS       Glass { albedo: pbr.albedo, ior: the record's, roughness: pbr.roughness }     (the guarded max(roughness, EPS))
 * and the reference's generic code around it: every model's sample draws one gen_r3() (the dimension budget of rpt_set_config is unchanged); next-event
 * estimation runs iff the sampled lobe is the diffuse reflection — always for Lambertian, never for Glass (lobes 1 and 3), so no light is sampled through
 * glass — and evaluates the surface's own evaluate / pdf (light_pick.rs:153-155); an emitter hit after a Glass bounce adds its emission (lib.rs:97) and the
 * carried light sample is not reset by one; `inside` is decided by the shading normal (bsdf.rs:131), after normal mapping.  The shared_structs layouts are
 * untouched: the records travel beside the material buffer.
 * rpt_set_material_models: after rpt_upload_scene, n_models == the scene's material count; callable between any two batches (it waits for what is enqueued);
 * leaves accumulator, rng, moments, statistics and shadow mode alone; rpt_upload_scene clears the records, rpt_set_config keeps them.  (NULL, 0): every
 * material PBR again.  RPT_EINVAL, with the context and its records as they were, for a model above 2, an ior that is not finite or not above 0 on a GLASS
 * record (ignored on the others), a count that is not the scene's, a call before a scene.  While every record is PBR, or none is set, the kernels launched are
 * the ones launched without this call.  `reserved` is ignored.
 * rpt_material_models: the records as set (n_out = 0: none), out nullable, capacity in records.
 * The denoiser's guides (rpt_read_guides) are first-hit guides by default: a glass pixel's guide is the glass surface — kind 1, albedo what the BSDF carries
 * (get_pbr_bsdf's).  rpt_set_guides_through_glass (with the denoiser, below) makes them follow glass to the surface seen through it.
 * Not carried: by rpt_world_save's .rptscene cache and by the host mirror rpt_trace_gpu (rpt_host.h). */
enum { RPT_MODEL_PBR = 0, RPT_MODEL_LAMBERTIAN = 1, RPT_MODEL_GLASS = 2 };
typedef struct rpt_material_model { uint32_t model; float ior; uint32_t reserved[2]; } rpt_material_model;
int rpt_set_material_models(rpt_ctx *ctx, const rpt_material_model *models, size_t n_models);  /* NULL, 0: all PBR */
int rpt_material_models(rpt_ctx *ctx, rpt_material_model *out, size_t capacity, size_t *n_out);
int rpt_multi_set_material_models(rpt_multi *m, const rpt_material_model *models, size_t n_models);   /* on every rank */
/* Absorbing glass: per-material Beer-Lambert attenuation.  Opt-in; no reference equivalent (Glass::sample's only colour is `spectrum = albedo`, once per
 * refracting interface, bsdf.rs:165: a thick block and a thin pane of one material come out the same colour).  One record per material beside the model
 * records: sigma, the absorption per unit scene length, r g b.  The rule, for closed, non-nested glass — a segment that ARRIVES at a Glass surface from the
 * inside has travelled through that glass:
 *   where    in the surface stage, at the hit (t, triangle) of an extension ray, whichever bounce it is, after the emission branch (lib.rs:86-108) has NOT
 *            ended the path
 *   iff      the material's model is RPT_MODEL_GLASS and dot(normal, view) < 0, with normal the very vector handed to Glass::sample — the shading normal after
 *            normal mapping, un-normalised (lib.rs:125) — and view = -ray_direction
 *   what     T_c = exp(-(sigma_c * t)), c = x, y, z: an f32 product, negated, through the deterministic, correctly rounded exp of csrc/rpt_math.h (rptm::expr);
 *            throughput = throughput * T, before the sample's own throughput = throughput * (spectrum / pdf)         (csrc/k_volume.h vol_transmit)
 * Nothing else changes: the draws and their dimensions, Glass::sample, next-event estimation (never for Glass), the roulette — which sees the attenuated
 * throughput as it sees any other — and the ray counts.  sigma_c == 0 gives exp(-0) = 1 and leaves that channel bit for bit; at the last bounce nothing reads
 * the throughput; an emissive Glass material ends the path before the rule applies.
 * Limits: the segment is attributed to the glass it ENDS on — one that ends on a non-glass object embedded in the glass, on an emitter, or in the sky through
 * an open mesh is not attenuated; there are no nested dielectrics; a single-sided Glass sheet reads "inside" from its back and attenuates by the distance to
 * the previous vertex, so volumes belong on closed meshes; the camera may start inside.  The denoiser's guides are unchanged: with
 * rpt_set_guides_through_glass the chain's albedo does not carry T (demodulation then leaves a smooth thickness term in the filtered image).
 * rpt_set_material_volumes: the life cycle of rpt_set_material_models — after rpt_upload_scene, n == the scene's material count; callable between any two
 * batches (it waits for what is enqueued); leaves accumulator, rng, moments, statistics, shadow mode, lens and guides alone (the guides are NOT marked stale);
 * rpt_upload_scene clears the records, rpt_set_config keeps them.  (NULL, 0): none.  Independent of the order in which it and rpt_set_material_models are
 * called: a record on a material that is not Glass is stored and ignored.  RPT_EINVAL, the message naming the record, with the context and both record sets
 * as they were, for a sigma channel that is negative, NaN or infinite, reserved != 0, a count that is not the scene's, NULL with n != 0 or the reverse, a call
 * before a scene.  With no records, with every sigma zero or with no Glass material the kernels launched are the ones launched without this call.
 * rpt_material_volumes: the records as set (n_out = 0: none), out nullable, capacity in records.
 * Not carried: by rpt_world_save's .rptscene cache and by the host mirror rpt_trace_gpu (rpt_host.h). */
typedef struct rpt_material_volume { float sigma[3]; uint32_t reserved; } rpt_material_volume;   /* absorption per unit scene length, r g b */
int rpt_set_material_volumes(rpt_ctx *ctx, const rpt_material_volume *volumes, size_t n);   /* NULL, 0: none */
int rpt_material_volumes(rpt_ctx *ctx, rpt_material_volume *out, size_t capacity, size_t *n_out);
int rpt_multi_set_material_volumes(rpt_multi *m, const rpt_material_volume *volumes, size_t n);   /* on every rank */
/* Punctual lights: point, spot and directional (glTF's KHR_lights_punctual), sampled by next-event estimation.  Opt-in; no reference equivalent (its only
 * emitters are emissive triangles — the alias table of light_pick.rs — and the sky).  One record per light, 64 bytes.  The lights act ONLY inside
 * sample_direct_lighting: NEE modes 1 and 2, at a bounce whose sampled lobe is the diffuse reflection.  A delta light cannot be met by a BSDF sample, so with
 * nee = 0 the lights add nothing and the kernels launched are the ones launched without this call.
 * Shares: with n lights the effective share q of the first light draw is 1 when the scene's table is the sentinel (no emissive triangle; pick_share is then
 * ignored), else pick_share, which must lie in (0, 1) exclusive; q = 0 when n = 0.
 * The four draws l1, l2, p1, p2 of light_pick.rs are made exactly when NEE runs and there is a mesh light or a punctual light: no dimension moves and
 * rpt_set_config's budget is unchanged.
 *   l1 < q   a punctual light j = min(f2u32_sat((l1 / q) * (float)n), n - 1), with pick pdf q / (float)n
 *   else     u = (l1 - q) / (1 - q) takes l1's place in the reference's alias pick (an over-run is clamped and counted as it is without lights) and
 *            light_pick_pdf becomes light_pick_pdf * (1 - q), in the light sample and in the carried MIS term of calculate_bsdf_mis_contribution alike.
 *            Over the sentinel table (q = 1) the only such draw is l1 == 1.0: nothing is picked, nothing evaluated and nothing counted.
 * Every quotient is an IEEE f32 division; with q = 0 this is the arithmetic without lights bit for bit (u = l1, the pdf times 1.0f).
 * The unoccluded term of a punctual pick (csrc/k_punctual.h punctual_sample states the f32 operation order):
 *   point, spot   v = position - hit, d = |v|, L = v / d; shadow ray from hit + L * EPS with max_t = d - 2 EPS, as the reference's; E = intensity * (spot / (d * d));
 *                 spot = 1 for a point light, and for a spot light a = clamp(dot(direction, -L) * angle_scale + angle_offset, 0, 1), spot = a * a
 *   directional   L = -direction, max_t = 1e6, E = intensity
 *   then          attenuation and bsdf_pdf are the surface's own diffuse evaluate / pdf (Lambertian::evaluate for a Lambertian record); if bsdf_pdf > 0:
 *                 direct = (attenuation * E) / pick_pdf — the weight is 1 in BOTH NEE modes — and contribution = throughput * direct
 * The elision rule is unchanged (a mask_nan term of zero: the ray is not queued); rpt_stats.shadow_rays and shadow_rays_elided count a punctual pick as they
 * count any NEE evaluation.  In MIS mode a punctual pick writes the carry "no triangle": an emitter met by the next BSDF sample then adds nothing, which is
 * the reference's one-sample rule (a BSDF hit counts only on the picked light, divided by that pick's pdf) and keeps the estimator unbiased.
 * Limits: no light is sampled through Glass (NEE never runs there): a glass object casts an opaque shadow from these lights and there are no caustics; no light
 * radius, so no soft shadows; no `range` attribute; the denoiser's guides are unchanged; the lights are not in rpt_world_save's .rptscene cache and not in the
 * host mirror rpt_trace_gpu.  glTF gives point and spot intensities in candela and directional ones in lux (683 lm/W): scaling to scene units is the caller's.
 * rpt_set_punctual_lights: callable after rpt_upload_scene, between any two batches (it waits for what is enqueued); cleared by rpt_upload_scene, kept by
 * rpt_set_config; the caller resets the accumulator, as for the lens; n <= 65535; (NULL, 0): none.  RPT_EINVAL, with the context and the lights as they were
 * and the message naming the record, for a type above 2; a non-finite position, direction or intensity; a negative intensity; a direction with
 * |len^2 - 1| > 1e-3 on a spot or directional record; a non-finite angle_scale or angle_offset; reserved != 0; NULL with n != 0 or the reverse; a pick_share
 * outside (0, 1), or NaN, while the scene has emissive triangles (and n != 0); a call before a scene.
 * rpt_punctual_lights: the records as set (n_out = 0: none) and the effective share q; out and effective_share_out nullable, capacity in records.
 * Checked: the device against a CPU restatement of the rule word for word; that restatement against an independent float64 reading of this text within
 * 8 x 1.714e-3 relative per sample, measured 0.03-0.13 % of the samples flagged as undecidable against a cap of 1 % (tests/f64_lights.py).  Measured on one MI355X, 32-spp MIS batches
 * (profiles/r23_punctual_lights.txt): the variant with no lights costs x 1.002 (DarkCornell 1024^2, 18.69 -> 18.72 ms) and x 1.009 (VeachMIS 1080p,
 * 28.41 -> 28.66 ms) of a batch; a context without lights launches what it launched before. */
enum { RPT_LIGHT_POINT = 0, RPT_LIGHT_SPOT = 1, RPT_LIGHT_DIRECTIONAL = 2 };
typedef struct rpt_punctual_light {
    uint32_t type;
    float position[3];      /* point, spot; ignored for directional */
    float direction[3];     /* spot, directional: the way the light shines, unit length, used AS GIVEN */
    float intensity[3];     /* point/spot: radiant intensity r g b (per steradian); directional: irradiance on a surface facing the light */
    float angle_scale, angle_offset;   /* spot: glTF's 1 / max(0.001, cos inner - cos outer) and -cos outer * scale */
    uint32_t reserved[4];   /* 0 */
} rpt_punctual_light;
int rpt_set_punctual_lights(rpt_ctx *ctx, const rpt_punctual_light *lights, size_t n, float pick_share);  /* NULL, 0: none */
int rpt_punctual_lights(rpt_ctx *ctx, rpt_punctual_light *out, size_t capacity, size_t *n_out, float *effective_share_out);
int rpt_multi_set_punctual_lights(rpt_multi *m, const rpt_punctual_light *lights, size_t n, float pick_share);   /* on every rank */
/* Thin-lens camera.  Opt-in; the reference's camera is a pinhole with a fixed 90 degree HORIZONTAL field of view (kernels/src/lib.rs:38-51) and
 * rpt_tracing_config carries a position and two angles only.  The lens replaces lib.rs:38-51 and nothing else of trace_pixel (csrc/k_lens.h states the f32
 * operations): the film coordinates are scaled by tan_half_fov before the direction is normalized, and with aperture_radius > 0 the ray leaves a point of
 * the lens disk — radius aperture_radius, in the camera's x-y plane — towards the point where the pinhole ray meets the plane focus_distance in front of the
 * camera.  The lens sample comes from the two entries of the reference's LDS table that no path reads (0 and 31), so every later draw of a path stays on its
 * dimension; entry 31 is read by a configuration that needs all 31 dimensions, hence: aperture_radius > 0 with such a configuration is RPT_ECONFIG, from
 * whichever of rpt_set_config / rpt_set_camera_lens comes second (the first one's setting stays).
 * The lens is INACTIVE iff tan_half_fov == 1.0f && aperture_radius == 0.0f, whatever the focus: the kernels launched and every output are then what they are
 * without this call.  An active lens needs two slots per pixel (paths are restarted by the completion kernel only): a context held to one
 * (rpt_set_samples_in_flight(ctx, 1), an image too large for two) refuses to render with RPT_EINVAL and says so.
 * rpt_set_camera_lens: holds from the next render call, like the camera fields of rpt_set_config: the CALLER resets the accumulator (rpt_reset); the denoiser's
 * guides are rebuilt at their next use (through the pixel centre and the LENS CENTRE: sharp whatever the aperture; the filters' plane term follows the field of
 * view).  Refused with RPT_EINVAL while an asynchronous batch is pending (rpt_wait first), for a tan_half_fov that is not finite or not above 0, an
 * aperture_radius that is negative or not finite, with aperture_radius > 0 a focus_distance that is not finite or not above 0, and reserved != 0 — the
 * message names the reason, the lens stays.  NULL: the default.  Survives rpt_set_config and rpt_upload_scene.
 * rpt_denoise_temporal under tan_half_fov != 1 is refused (RPT_EINVAL): its reprojection is the inverse of the reference's camera.
 * Not carried by the host mirror rpt_trace_gpu (rpt_host.h). */
typedef struct rpt_camera_lens {
    float tan_half_fov;     /* tangent of half the HORIZONTAL field of view; 1.0 = the reference's camera */
    float aperture_radius;  /* lens radius in scene units; 0 = pinhole */
    float focus_distance;   /* distance of the plane in focus along the view axis; read only when aperture_radius > 0 */
    uint32_t reserved;      /* 0 */
} rpt_camera_lens;
void rpt_camera_lens_default(rpt_camera_lens *out);          /* {1, 0, 1, 0} */
int rpt_set_camera_lens(rpt_ctx *ctx, const rpt_camera_lens *lens);   /* NULL = default */
int rpt_camera_lens_get(rpt_ctx *ctx, rpt_camera_lens *out);
int rpt_multi_set_camera_lens(rpt_multi *m, const rpt_camera_lens *lens);   /* on every rank */
/* How the LAST extension rays of a batch of known length are walked when the configuration has no NEE.  At bounce max_bounces - 1 the reference reads three
 * things off intersect_nearest (kernels/src/lib.rs:62-109): a miss adds the sky, a hit on the front of an emissive triangle adds its emission, any other hit
 * adds nothing — so a ray that passes the Moller-Trumbore test of no emissive triangle only has to answer "hit or miss", which the reference's own walk
 * answers at its FIRST accepted triangle (intersection.rs:195-203), in any visiting order.  mode_out: 0 the plain walk (more than four emissive triangles, a
 * scene that does not live in LDS, RPT_LAST_BOUNCE_HIT_OR_MISS=0); 1 those rays stop at their first accept, near child first; 2 / 3 / 4 fixed order over a
 * copy flipped so that the more opaque / the smaller / the more-opaque-per-node child comes first — chosen at rpt_upload_scene by the node visits of
 * synthetic rays (visits_out[4]: near first, then the three rules; csrc/shadow_order.h choose_last_order).  The image is the same in every mode. */
int rpt_last_bounce_order(rpt_ctx *ctx, uint32_t *mode_out, uint32_t *n_emissive_triangles_out, double *visits_out /* [4], nullable */, uint32_t *probe_rays_out,
                          double *probe_ms_out);

/* --- denoise (the third step of the reference's read-back: read, divide by the sample count, DENOISE — src/trace.rs:197-213, the "Denoise" checkbox of
 * src/app.rs:245-249, there OIDN) --------------------------------------------------------------------------------------------------------------------
 * Opt-in, after the accumulator; the wavefront pipeline, its parity statements and bench.py's figures are not touched.  Two parts (csrc/k_denoise.h):
 *   guides   the first hit of the ray through every pixel's centre (camera_ray with the jitter replaced by (0.5, 0.5)), for the WHOLE image whatever the
 *            context's partition: kind 0 miss / 1 surface / 2 emitter (material.emissive.xyz != 0, either face); albedo = what get_pbr_bsdf uses
 *            (bsdf.rs:355-361; (1,1,1) for kinds 0 and 2); the normalised shading normal of lib.rs:125-141 ((0,0,0) on a miss or where it is zero / not
 *            finite); depth = trace_result.t (1e6 on a miss); position = ro + rd * depth.  Cached on the context: rebuilt at the first use after
 *            rpt_set_config or rpt_upload_scene, not per call.  These rays are not counted in rpt_stats.  rpt_read_guides hands them out — also the
 *            albedo / normal auxiliary images a host-side OIDN takes.
 *   filter   an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over mean = sum / samples: `iterations` passes of 5 x 5 taps at step 2^i,
 *            weights from normal, plane distance and colour, between pixels of the same kind only; with `demodulate` the mean is divided by max(albedo, 0.01)
 *            first and multiplied back at the end; then tonemap operator 0..6 as rpt_resolve.  iterations = 0 is exactly rpt_resolve(tonemap_op).
 *            Deterministic, f32, no atomics: the device result equals the host build of the same header (rpt_debug_denoise_host) bit for bit and does not
 *            depend on the number of GPUs.  The formulas: csrc/k_denoise.h dn_filter_pixel, DESIGN.md "Denoiser".
 * rpt_denoise synchronises by itself and is synchronous on return; it leaves the accumulator, the rng, the counters and the shadow mode untouched and may be
 * called between any two batches.  source:
 *   RPT_DENOISE_ACCUM     the context's own accumulator; needs a partition of one rank (else RPT_EINVAL).
 *   RPT_DENOISE_GATHERED  the image of the last gather, on rank 0 of a communicator (rpt_comm_init_local included): waits for that gather, uses its sample
 *                         count, and filters on the gather's stream — a batch enqueued since keeps rendering.  RPT_EINVAL on other ranks or before any gather.
 * RPT_EINVAL also for iterations > 6, normal_power_log2 > 10, a negative or non-finite sigma, tonemap_op > 6 and zero samples; the context stays usable.
 * out_rgb: width*height*3 floats, row-major.  report (nullable): device_ms = the filter (pre-pass + passes, HIP events), guides_ms = the guide build of this
 * call (0 when cached), guides_rebuilt 0 / 1.  There is no environment variable for any of it. */
typedef struct rpt_denoise_params {
    uint32_t iterations;          /* 0..6 passes, step 2^i */
    uint32_t normal_power_log2;   /* 0..10: the normal weight max(0, n_p . n_q) is squared this many times */
    float    sigma_color;         /* colour edge-stopping width, halved every pass; 0 = no colour term */
    float    sigma_plane;         /* plane-distance width in pixel footprints */
    uint32_t demodulate;          /* filter mean / max(albedo, 0.01) */
    uint32_t reserved[3];
} rpt_denoise_params;

typedef struct rpt_denoise_report {
    double   device_ms;
    double   guides_ms;
    uint32_t guides_rebuilt;
    uint32_t pixels_clamped;      /* pixels the firefly clamp of rpt_denoise_variance / rpt_denoise_temporal changed; 0 while it is off, and from rpt_denoise */
} rpt_denoise_report;

enum { RPT_DENOISE_ACCUM = 0, RPT_DENOISE_GATHERED = 1 };

/* the parameters with the lowest summed error against converged images of the three shipped scenes (profiles/r11_denoise_quality.txt) */
void rpt_denoise_params_default(rpt_denoise_params *out);
int rpt_denoise(rpt_ctx *ctx, uint32_t source, const rpt_denoise_params *params /* NULL = defaults */, uint32_t tonemap_op, float *out_rgb,
                rpt_denoise_report *report /* nullable */);
/* width*height entries each, row-major; every pointer nullable.  Builds the guides if they are stale. */
int rpt_read_guides(rpt_ctx *ctx, float *albedo_rgb, float *normal_xyz, float *depth, float *position_xyz, uint32_t *kind);
/* waits, gathers as rpt_multi_read_accum does, and denoises on rank 0 */
int rpt_multi_denoise(rpt_multi *m, const rpt_denoise_params *params, uint32_t tonemap_op, float *out_rgb, rpt_denoise_report *report);

/* --- guides that follow glass to the surface seen through it ---------------------------------------------------------------------------------------------
 * Opt-in, default off: with max_interfaces = 0 the guides, the kernels that build them and their bytes are what they were.  A first-hit guide of a pixel that
 * looks through a pane or a lens is the glass surface — kind 1, the glass's tint, its smooth normal, its depth, all nearly constant across the pane — while
 * the radiance there is an image of what lies behind: the passes find no edge and blur it, demodulation divides by the tint instead of the albedo behind, and
 * the firefly clamp's window mixes an emitter seen through glass with the wall beside it.
 * With K = max_interfaces in 1..8 the guide of a pixel is the end of a deterministic chain (csrc/k_guides_glass.h dn_glass_step).  From the
 * centre ray, with A = (1,1,1), L = 0, m = 0, per nearest hit (t, triangle) of the current ray (ro, rd):
 *   miss                                kind 0, normal (0,0,0), albedo A, L += 1e6; done
 *   hit                                 shaded as the first-hit guide: n = the normalised shading normal (zero if not finite), a = the albedo ((1,1,1) on an
 *                                       emitter), L += t
 *   emitter, record not Glass, no records    that kind, n, albedo A * a; done
 *   Glass and m == K, or n == 0         the budget is exhausted: kind 1, n, albedo A * a — the glass surface itself; done
 *   Glass and m < K                     view = -rd; inside = n . view < 0; n' = inside ? -n : n; (in_ior, out_ior) = inside ? (ior, 1) : (1, ior); c = view . n';
 *                                       F = f0 + (1 - f0) (1 - max(c, 0))^5, f0 = ((in_ior - out_ior) / (in_ior + out_ior))^2   (Glass::sample at zero
 *                                       roughness, bsdf.rs:128-165, the microsurface normal = n);
 *                                       F > 0.5: dir = normalize(2 |c| n' - view), A unchanged;
 *                                       else eta = in_ior / out_ior, dir = normalize((eta c - signum(c) sqrt(max(1 + eta (c c - 1), 0))) n' - eta view), A = A * a
 *                                       (the reference's clamped root: total internal reflection degrades as the tracer's does);
 *                                       ro = hit + dir * 0.001, rd = dir, m += 1; a dir that is not finite counts as an exhausted budget
 * The chain uses the NORMALISED shading normal where the tracer hands its BSDF the un-normalised one (lib.rs:125): it is a guide, not a sample.  L sums the
 * hit distances only, not the 0.001 shifts of the origin.  The records of the final values, (ro0, rd0) the centre ray:
 *   normal, albedo = A * a (A on a miss), kind in {0, 1, 2} as before, depth = L, position = ro0 + rd0 * L
 * — the point at optical path length L UNFOLDED ALONG THE PRIMARY RAY, not the hit point: it lies on the pixel's own ray, so the temporal reprojection stays
 * self-consistent and depth stays the distance the footprint grows with.  Behind a flat pane it differs from the true point by the pane's small lateral
 * shift; through a lens the unfolded positions are distorted, the plane term then rejects more taps and the filter is weaker there, not wrong.
 * A pixel whose chain meets no glass, and every pixel while no record is Glass, has the first-hit guide byte for byte (then the first-hit kernels are the ones
 * launched).  The filters, the temporal kernel and the firefly clamp are unchanged: they read the same records.
 * Cost: one walk of the whole image, then one walk per further round of only the rays still inside glass, compacted in ascending ray order; at most K + 1.
 * rpt_set_guides_through_glass   0..8; above: RPT_EINVAL, the setting stays.  Callable at any time; a change marks the guides stale.  While it is above 0,
 *                                rpt_set_material_models marks them stale too.  Survives rpt_upload_scene and rpt_set_config.  rpt_multi_: on every rank.
 * rpt_guides_info_get            the setting and the last build: rounds = walks made (0 before any build), rays[r] = rays walked in round r,
 *                                pixels_through_glass = pixels whose chain crossed at least one interface, pixels_exhausted = pixels whose chain ended on a
 *                                glass surface (budget, zero normal or a direction that is not finite). */
typedef struct rpt_guides_info {
    uint32_t max_interfaces;
    uint32_t rounds;
    uint32_t rays[9];
    uint32_t pixels_through_glass;
    uint32_t pixels_exhausted;
    uint32_t reserved[3];
} rpt_guides_info;
int rpt_set_guides_through_glass(rpt_ctx *ctx, uint32_t max_interfaces);     /* default 0 */
int rpt_guides_through_glass(rpt_ctx *ctx, uint32_t *max_interfaces_out);
int rpt_guides_info_get(rpt_ctx *ctx, rpt_guides_info *out);
int rpt_multi_set_guides_through_glass(rpt_multi *m, uint32_t max_interfaces);

/* --- per-pixel sample moments, noise estimate, render to a noise target (no reference equivalent: `samples` is the only progress figure of the reference's
 * TracingState, src/trace.rs:40-50) ------------------------------------------------------------------------------------------------------------------
 * Opt-in; the default pipeline, its parity statements and bench.py's figures are not touched, and the image does not depend on it, bit for bit.
 * With moments on a context keeps one more float4 per owned pixel beside the accumulator, updated once per finished sample, in sample order, with the radiance r
 * that the accumulator gets (csrc/k_moments.h, f32, no contraction):
 *     Y = (0.2126f * r.x + 0.7152f * r.y) + 0.0722f * r.z
 *     m.x += Y          sum of luminance                  m.z += 1          samples since the moments were last zeroed
 *     m.y += (Y * Y)    product rounded, then added       m.w  = Y > m.w ? Y : m.w     the brightest sample (a NaN never enters)
 * The f32 sum order is part of the result, as for the accumulator: the record equals a sequential restatement word for word (tests/test_gpu_moments.py).
 * They are added by a second completion kernel (csrc/k_complete.h k_complete_moments) that is launched instead of k_complete while moments are on; every
 * other kernel is the same.  A sample must pass through that kernel, so a render call with moments on keeps at least two slots per pixel busy (a
 * one-sample call uses slot 0 of 2); a context that can only have one — after rpt_set_samples_in_flight(ctx, 1), or with an image too large for two slots
 * per pixel — refuses to render with moments on (RPT_EINVAL, the message says so; rpt_set_samples_in_flight(ctx, 0) or rpt_set_moments(ctx, 0) is the way
 * out) and stays usable.
 * Cost, DERIVED, NOT YET MEASURED on a device (tools/moments_probe.py --cost is the measurement; profiles/r12_moments.txt says what has been run): the
 * completion reads 32 x 16 B of radiance and moves 32 B of accumulator per pixel and 32-spp batch; the moments add 32 B (+6 % of that stage's traffic) and four VALU
 * operations per sample; the stage is about 2 % of a batch, so a batch should move by about 0.1 %.  With moments off the completion kernel is the same kernel,
 * instruction for instruction.
 *
 * rpt_set_moments   may be called between any two batches; synchronises.  Turning it on allocates and zeroes the record (on while on: nothing happens),
 *                   turning it off frees it.  Leaves the accumulator, the rng, rpt_stats and the shadow mode untouched.
 * The moments are zeroed when they are turned on, by rpt_reset, and by every configuration change that invalidates the accumulator (a resize,
 * rpt_set_partition, rpt_set_samples_in_flight).  rpt_reset with accum_init resumes the accumulator but NOT the moments: m.z then counts only the samples
 * rendered since, while the accumulator's .w continues from samples_init.
 *
 * noise_rel(m), with n = m.z: +inf if n < 2 or m.x or m.y is not finite; else
 *     mean = m.x / n;  ss = m.y - (m.x * m.x) / n;  v = ss / (n * (n - 1));  sem = sqrt(v > 0 ? v : 0);  rel = sem / (|mean| + 0.01f)
 * — the standard error of the pixel's mean luminance relative to that mean, with a floor that keeps black pixels finite.
 * A LIMIT OF EVERY EMPIRICAL-VARIANCE CRITERION: a pixel whose samples so far were all equal has rel = 0 and looks converged.  On DarkCornell without NEE
 * at 100 x 70, 6453 of 7000 pixels have zero variance after 8 samples (most have not seen the light yet) and only 507 are above any threshold; after 128
 * samples 4511 are above 0.1.  That is what rpt_noise_target.min_samples is for (DESIGN.md "Moments and noise estimate").
 *
 * rpt_read_moments  width*height float4, row-major; rpt_read_noise: noise_rel of every pixel, width*height floats.  Both synchronise and un-tile as
 *                   rpt_read_accum does; other ranks' pixels are zero.
 * rpt_noise_count   pixels = the pixels this context owns, measured = those with n >= 2, above = the measured ones with !(rel <= threshold).  One kernel
 *                   with integer atomics behind whatever is enqueued, 24 bytes read back.  Integers: order-independent and additive over ranks —
 *                   rpt_multi_noise_count is the sum over its contexts; a process-per-GPU caller (rpt_comm_*) all-reduces the three integers itself
 *                   (nothing is added to the gather).  threshold: >= 0, +inf allowed.
 * rpt_render_to_noise   turns moments on if they are off (and leaves them on), then renders batches of batch_samples through rpt_render_async, the last one
 *                   clipped so that max_samples is not exceeded; after each batch, once at least min_samples have been rendered by this call, it counts
 *                   (same stream, one small read-back per batch) and stops with converged = 1 when measured == pixels && above <= max_above, or with
 *                   converged = 0 at max_samples.  The accumulator is bit for bit that of plain rendering of samples_rendered samples: the image never
 *                   depends on how samples are split into calls.  counts = the last count; ms = host clock over the whole call.
 *                   RPT_EINVAL for batch_samples == 0, max_samples < min_samples, a negative or NaN threshold.
 * rpt_multi_*       the same on every rank; rpt_multi_read_moments merges the ranks' images on the host (the pixels are disjoint; off the hot path) — or,
 *                   with rpt_multi_gather_set_moments(m, 1), gathers if nothing is gathered and is one copy of the gathered record from rank 0.
 * RPT_EINVAL from the read and count entry points while moments are off, and for null pointers. */
int rpt_set_moments(rpt_ctx *ctx, uint32_t on);      /* default 0 */
int rpt_moments(rpt_ctx *ctx, uint32_t *on_out);
int rpt_read_moments(rpt_ctx *ctx, float *out_xyzw); /* width*height float4, row-major; other ranks' pixels zero */
int rpt_read_noise(rpt_ctx *ctx, float *rel_out);    /* width*height floats, row-major; other ranks' pixels zero */

typedef struct rpt_noise_counts { uint64_t pixels, measured, above; } rpt_noise_counts;
int rpt_noise_count(rpt_ctx *ctx, float threshold, rpt_noise_counts *out);

typedef struct rpt_noise_target {
    float threshold;
    uint32_t min_samples, max_samples, batch_samples;
    uint64_t max_above;
} rpt_noise_target;
typedef struct rpt_noise_result {
    uint32_t samples_rendered, converged;
    rpt_noise_counts counts;
    double ms;
} rpt_noise_result;
int rpt_render_to_noise(rpt_ctx *ctx, const rpt_noise_target *target, rpt_noise_result *out);

int rpt_multi_set_moments(rpt_multi *m, uint32_t on);
int rpt_multi_read_moments(rpt_multi *m, float *out_xyzw);
int rpt_multi_gather_set_moments(rpt_multi *m, uint32_t on);   /* rpt_gather_set_moments on every rank ("the moments record ... inside the gather", above) */
int rpt_multi_noise_count(rpt_multi *m, float threshold, rpt_noise_counts *out);
int rpt_multi_render_to_noise(rpt_multi *m, const rpt_noise_target *target, rpt_noise_result *out);

/* --- variance-guided denoise: the filter of rpt_denoise with one more edge-stopping term, driven by the per-pixel moments (Schied et al. 2017) ---------
 * Opt-in, a second entry point: rpt_denoise, its kernels and its defaults are what they were.  From a moments record m of a pixel (n = m.z) the pre-pass takes
 * the empirical variance of the pixel's MEAN luminance (csrc/k_moments.h mo_variance_of_mean; the square of noise_rel's standard error, not divided by the mean):
 *     v = max(0, m.y - (m.x * m.x) / n) / (n * (n - 1))          UNKNOWN, written +inf, if n < 2 or m.x or m.y is not finite
 * and, where the mean is demodulated, divides it by Ya * Ya, Ya = the luminance of max(albedo, 0.01): v is in the units of the filtered image's luminance,
 * squared.  The mean itself is rpt_denoise's (by the uniform count, or by every pixel's own .w while rpt_counts_uniform is 0).  Pass i, centre p
 * (csrc/k_denoise.h dn_filter_pixel_var, DESIGN.md "Denoiser"):
 *     vbar_p = the 3 x 3 Gaussian {1/4, 1/2, 1/4}^2 of the pass's input variance around p (distance 1 at every step) over the taps inside the image, of p's
 *              kind and of known variance, divided by the kernel weights used; unknown if there is no such tap
 *     d_l    = |Y(e_p) - Y(e_q)| / (sigma_variance * sqrt(vbar_p) + 1e-6)     added to d_x + d_c of tap q, if sigma_variance != 0 and vbar_p is known
 *     v_out  = sum(w^2 v_q) / sum(w)^2 over the joined taps of known variance, the centre included; known iff the centre's was
 * Every other rule is rpt_denoise's.  With sigma_variance == 0, or where vbar_p is unknown (every record unmeasured, say), no term is added and the image is
 * rpt_denoise(base)'s bit for bit.  A pixel whose neighbourhood has zero variance — all samples equal, which an empirical variance reads as converged —
 * joins only taps of (almost) equal luminance: sigma_variance * 0 + 1e-6 is the width.  sigma_variance = +inf is allowed: where vbar_p > 0 the width is
 * +inf and d_l = 0; where vbar_p == 0 the width is inf * 0 = NaN, d_l and w are NaN, and by rpt_denoise's rule (a weight that is not > 0 never joins) no
 * tap joins: such a pixel passes through unchanged.
 * After rpt_reset with accum_init the moments count only the samples rendered since, while the accumulator continues: v is then the variance of the mean
 * of the samples SINCE THE RESET, a larger figure than that of the whole accumulator's mean.
 *
 * moments_xyzw == NULL   the context's own record, on the device, no host trip.  With RPT_DENOISE_ACCUM; RPT_EINVAL while moments are off.  With
 *                        RPT_DENOISE_GATHERED only under rpt_gather_set_moments(ctx, 1): the gathered record, on the device, no host trip.
 * moments_xyzw != NULL   a width*height float4 row-major image — what rpt_read_moments / rpt_multi_read_moments return — uploaded for this call; with either
 *                        source.  The way a process-per-GPU caller filters a gathered image while moments are not part of the gather (rpt_gather_set_moments off).
 * out_variance (nullable, width*height floats): the last pass's v_out, in the filter's units (demodulated where demodulation was applied; iterations == 0:
 *                        the pre-pass's v, never demodulated); unknown = +inf.
 * RPT_EINVAL for a negative or NaN sigma_variance, a null out_rgb, and for everything rpt_denoise refuses; the context stays usable.  Synchronous on
 * return; leaves the accumulator, the rng, the moments, rpt_stats, the shadow mode and the cached guides untouched.
 * rpt_multi_denoise_variance merges the ranks' records on the host as rpt_multi_read_moments does (OFF THE HOT PATH: a read-back and an upload of 16 bytes
 * per pixel on every call), gathers as rpt_multi_denoise does, and filters on rank 0.  With rpt_multi_gather_set_moments(m, 1) it gathers if nothing is
 * gathered and filters by the gathered record: no per-rank read-back, no host merge, no upload; the result is the host merge's bit for bit.
 * Defaults: the lowest summed error of the grid of profiles/r14_denoise_variance_quality.txt.
 *
 * FIREFLY CLAMP (clamp_scale != 0; csrc/k_firefly.h ff_pixel, DESIGN.md "Denoiser").  The moments record's m.w is the luminance of the pixel's brightest sample.
 * Before the mean is demodulated, for a pixel p with mean c (radiance), count_p (its own .w while rpt_counts_uniform is 0, else the uniform count) and record m:
 *     Ya_q = the luminance of max(albedo_q, 0.01) where the passes demodulate, else 1;   b(q) = m_q.w / Ya_q
 *     B    = the largest b(q) over the taps q != p with |dx|, |dy| <= clamp_radius that are inside the image, of p's kind, hold m_q.z >= 1 and a finite b(q)
 *     L    = max(clamp_scale * B, clamp_floor) * Ya_p
 * p is clamped iff there is such a tap, m.z >= 1, m.z == count_p, m.x, m.y, m.w and L are finite, m.x > 0 and m.w > L; then, with w = m.w:
 *     x' = max(0, (m.x - w) + L),  y' = max(0, (m.y - w * w) + L * L),  rho = min(1, x' / m.x),  c' = c * rho,  m' = (x', y', m.z, L)
 * and the call runs unchanged on (c', m'): the variance of the mean comes from m', and rpt_denoise_temporal blends — and keeps as history — c' and m', so a
 * spike is clamped before it can enter the history.  A record that does not count what the accumulator counts (after rpt_reset with accum_init, or a
 * caller's image with another m.z) is left alone.  rpt_denoise_report.pixels_clamped counts the clamped pixels (one integer atomic per wave).
 * The accumulator, the rng and the moments record are only read; with clamp_scale == 0 the other two words are ignored, the kernels launched are the ones
 * launched before the fields existed, and so are the bytes returned.  Plain rpt_denoise has no record and therefore no clamp.
 * LIMITS: only a pixel's ONE brightest sample is clamped; the removed part is assumed to have the pixel's mean chroma; two adjacent spikes of like size
 * shield each other; and the clamp is BIASED — it removes energy.  On the 8-spp oracle images, at clamp_scale 2 and clamp_radius 1, it removes 0.4 % (PBRTest),
 * 1.2 % (VeachMIS with NEE) and 1.4 % (DarkCornell with NEE) of the image's summed radiance, and 13.2 % of DarkCornell without NEE, where almost every lit
 * sample is rare; at 1 spp on that scene, clamp_scale 1 and clamp_radius 3, it is 61 % (profiles/r16_firefly_quality.txt, "lost").  It relaxes by itself as
 * samples grow, because the window then sees more of the rare events.  y' cancels where the spike dominated m.y: with u = 2^-24 and e_L the relative error of L
 * (9u where the passes demodulate, else u) its absolute error is at most D = u w^2 + u |m.y - w^2| + (2 e_L + u) L^2 + u y' — below 3 u w^2 where the spike
 * dominated and the limit is well below it (|m.y - w^2| <= w^2 / 4, L <= w / 4), up to 21 u w^2 where L is near w — and the variance of the mean is off by up to
 * D over n (n - 1).
 * DEFAULTS: the clamp ships OFF in rpt_denoise_var_params_default and rpt_temporal_params_default, so that a call which does not ask for it returns what it
 * returned before.  The grid of profiles/r16_firefly_quality.txt (rel-L2 against 1024-spp oracle images, four scenes) has its lowest summed ratio at
 * clamp_scale 2, clamp_radius 1 for rpt_denoise_variance at 8 spp (2.245 against 2.275 with the clamp off: little) and at clamp_scale 1, clamp_radius 3 for
 * rpt_denoise_temporal over an eight-view path at 1 / 2 / 4 spp (1.555 against 1.818; the scenes with NEE gain most, DarkCornell with NEE at 2 spp 0.085
 * against 0.169); the defaults carry those radii, so setting clamp_scale alone turns the recommended window on: clamp_scale 2 goes
 * with rpt_denoise_var_params_default's clamp_radius 1, clamp_scale 1 with rpt_temporal_params_default's clamp_radius 3.
 * RPT_EINVAL for a clamp_scale or clamp_floor that is negative, NaN or infinite, and for a clamp_radius outside 1..3 while clamp_scale != 0; the context
 * stays usable. */
typedef struct rpt_denoise_var_params {
    rpt_denoise_params base;      /* as rpt_denoise */
    float    sigma_variance;      /* width of the luminance term in standard errors; 0 = term off */
    float    clamp_scale;         /* firefly clamp: a pixel's brightest sample is held to clamp_scale x the brightest sample of its window; 0 = clamp off */
    float    clamp_floor;         /* ... and to no less than this (radiance; demodulated radiance where the passes demodulate) */
    uint32_t clamp_radius;        /* the window is (2 r + 1)^2 pixels without its centre, r = 1..3; read only while clamp_scale != 0 */
} rpt_denoise_var_params;
void rpt_denoise_var_params_default(rpt_denoise_var_params *out);
int rpt_denoise_variance(rpt_ctx *ctx, uint32_t source, const float *moments_xyzw /* nullable */, const rpt_denoise_var_params *params /* NULL = defaults */,
                         uint32_t tonemap_op, float *out_rgb, float *out_variance /* nullable, width*height */, rpt_denoise_report *report /* nullable */);
int rpt_multi_denoise_variance(rpt_multi *m, const rpt_denoise_var_params *params, uint32_t tonemap_op, float *out_rgb, float *out_variance,
                               rpt_denoise_report *report);

/* --- temporal reuse: rpt_denoise_variance with the previous view's history reprojected and blended in front of the passes ------------------------------
 * Opt-in, a third entry point: rpt_denoise, rpt_denoise_variance, their kernels and their defaults are what they were.  The reference zeroes the
 * accumulator whenever the camera moves and shows the unfiltered image of those frames (src/trace.rs:187-222); this call gives such a frame the samples and
 * the variance of the view before it.  The formulas: csrc/k_temporal.h tp_pixel, DESIGN.md "Denoiser".
 *
 * History (kept on the context, 56 bytes per pixel and slot, two slots, allocated at first use): per pixel the blended colour e_h in the filter's units
 * (demodulated where the passes demodulate), an f32 sample count N (0 = none) and the per-sample first and second luminance moments mu1, mu2, beside a copy
 * of the guide records and the camera of the view it was made under.  IT IS THE BLENDED IMAGE BEFORE THE PASSES, NOT THE FILTERED ONE.
 * Two slots: LAST, what the most recent call produced, and PREVIOUS, the history from before the current accumulator epoch.  An epoch ends at rpt_reset and at
 * whatever else invalidates the accumulator; the first call of a new epoch promotes LAST to PREVIOUS; every call of an epoch blends the current accumulator
 * with the same PREVIOUS (a second call after more samples does not count its own samples twice) and overwrites LAST.
 * The history is dropped (history_state = 2, the call runs without it) on a change of width or height, on rpt_upload_scene, and when the passes demodulate
 * (base.demodulate != 0 with base.iterations != 0) where the slot's did not or the reverse.  rpt_temporal_reset forgets and frees it; so do a resize and destroy.
 *
 * Per pixel p: its world position x_p is projected into the previous view (the pinhole camera inverted in closed form; misses by the rotation alone), the
 * four bilinear taps there join if they hold history (N > 0), are of p's kind and — for hits — pass  n_p . n_q >= normal_min  and
 * |n_p . (x_q - x_p)| / ((2 / width) t_p) <= plane_max  (footprints of p off its tangent plane); joined weights below 0.01 in sum: no history.  The taps'
 * weighted means e_r, mu1_r, mu2_r and N_r = min(weighted mean of N, max_history) blend with the current mean e_cur and moments record m (n_cur = m.z):
 *     T = N_r + n_cur,  e = (N_r e_r + n_cur e_cur) / T,  mu1 = (N_r mu1_r + m.x) / T,  mu2 = (N_r mu2_r + m.y) / T,
 *     v = max(0, mu2 - mu1 mu1) / (T - 1)    (unknown, +inf, if T < 2; divided by Ya^2 where demodulated)
 * and (e, v) goes through the unchanged passes of rpt_denoise_variance (`filter`).  A pixel without history — and every pixel of a call without a PREVIOUS
 * slot — is rpt_denoise_variance's bit for bit, colour and variance.  A current mean that is not finite passes through and leaves no history.
 *
 * moments_xyzw, out_variance, source: as rpt_denoise_variance.  out_history (nullable, width*height floats): T per pixel (> n_cur exactly where history
 * was reused).  rpt_multi_denoise_temporal: as rpt_multi_denoise_variance; the history lives on rank 0.
 * RPT_EINVAL for everything rpt_denoise_variance refuses, for a negative or NaN max_history or plane_max (+inf allowed) and for a normal_min that is NaN or
 * outside [-1, 1]; the context stays usable and its history is untouched.  Synchronous on return; leaves the accumulator, the rng, the moments, rpt_stats,
 * the shadow mode and the cached guides untouched.
 * Defaults: the lowest summed error of the grid of profiles/r15_temporal_quality.txt. */
typedef struct rpt_temporal_params {
    rpt_denoise_var_params filter;   /* the passes, and the firefly clamp in front of the blend: as rpt_denoise_variance */
    float    max_history;            /* cap on the reprojected sample count N_r; 0 = history never used */
    float    normal_min;             /* a history tap joins only if n_p . n_q >= normal_min */
    float    plane_max;              /* ... and |n_p . (x_q - x_p)| / ((2 / width) * t_p) <= plane_max  (footprints) */
    uint32_t reserved[5];
} rpt_temporal_params;
typedef struct rpt_temporal_report {
    rpt_denoise_report base;         /* device_ms includes the temporal kernel; pixels_clamped as rpt_denoise_variance */
    uint64_t pixels_with_history;    /* pixels whose N_r > 0 */
    uint32_t history_state;          /* 0 none yet, 1 used, 2 dropped by this call (resize / scene / demodulate changed) */
    uint32_t reserved;
} rpt_temporal_report;
void rpt_temporal_params_default(rpt_temporal_params *out);
int rpt_denoise_temporal(rpt_ctx *ctx, uint32_t source, const float *moments_xyzw /* nullable */, const rpt_temporal_params *params /* NULL = defaults */,
                         uint32_t tonemap_op, float *out_rgb, float *out_variance /* nullable, width*height */, float *out_history /* nullable, width*height */,
                         rpt_temporal_report *report /* nullable */);
int rpt_temporal_reset(rpt_ctx *ctx);
int rpt_multi_denoise_temporal(rpt_multi *m, const rpt_temporal_params *params, uint32_t tonemap_op, float *out_rgb, float *out_variance, float *out_history,
                               rpt_temporal_report *report);
int rpt_multi_temporal_reset(rpt_multi *m);

/* --- chosen pixels: masked passes, per-pixel sample counts to a noise target (no reference equivalent) --------------------------------------------------
 * Opt-in; a context that never makes a masked or adaptive call runs the same kernels as before, and bench.py's figures are not touched.
 * A sample depends only on its pixel's (x, y), its rng (n, offset) and the scene, and samples are added in sample order: a pixel that has received N samples
 * BY ANY ROUTE — uniform calls, masked passes, in any split — holds bit for bit what the reference holds after N samples (accumulator with .w = N, rng.n
 * advanced by N, moments).  tests/test_gpu_adaptive.py holds every case to that.
 * A masked pass (csrc/k_adaptive.h, rpt_adaptive.hip): a flag per owned pixel; the flagged pixels compacted in ascending pixel order (count per workgroup,
 * scan, scatter: the survivors keep the tile-major order and nothing depends on the order waves arrive in); their (pixel_xy, rng, accum, moments) copied
 * into compact arrays; the unchanged pipeline on those arrays, exactly as on a rank that owns that many pixels — with as many samples of a pixel in flight
 * as fit in the slots a whole-image call of this context may allocate (up to 256; rpt_set_samples_in_flight(n > 0) holds for a pass too), so a few thousand
 * pixels still fill the GPU; the records copied back, stream-ordered behind the batch.  The number of selected pixels comes back as one 4-byte read, the
 * pass's only synchronisation; nothing selected: nothing is launched, the call succeeds.  A pass whose batch has a known length (rpt_render_async) returns
 * once enqueued, otherwise it is synchronous; every read-out synchronises anyway.  A pass that selects EVERY owned pixel is the uniform call it amounts to.
 *
 * rpt_render_pixels   n_samples more samples for the owned pixels whose mask byte is non-zero (mask: width*height bytes, row-major; other ranks' pixels
 *                     ignored).  rpt_stats.samples grows by selected pixels x n_samples.
 * Sample counts then differ between pixels.  accum.w and rng.n carry each pixel's own count; rpt_read_accum's out_samples keeps reporting the samples EVERY
 * owned pixel received through uniform calls (a uniform rpt_render after a masked pass adds n to every pixel and to that figure).  rpt_counts_uniform:
 * 0 once a masked or adaptive pass has rendered for fewer than all owned pixels, 1 again after rpt_reset or whatever invalidates the accumulator.  While it
 * is 0, rpt_resolve and rpt_denoise(RPT_DENOISE_ACCUM) divide every pixel by its own .w (a pixel with .w == 0 resolves to 0); rpt_gather_async snapshots
 * the flag beside the sample count and rpt_denoise(RPT_DENOISE_GATHERED) / rpt_multi_denoise honour the snapshot (one process per GPU: the root snapshots
 * ITS flag — ranks that were masked differently must tell it; rpt_multi: any rank's).  While it is 1 both are the code and the results they always were.
 *
 * rpt_render_adaptive   per-pixel sample counts to a noise target.  Reuses rpt_noise_target and its refusals; turns moments on if they are off and leaves
 *                     them on.  Uniform phase: exactly min_samples for every pixel, in batches of at most batch_samples (rpt_render_async).  Then, before
 *                     each masked pass, one kernel selects the pixels with
 *                         !(noise_rel(m) <= threshold) && m.z + batch_samples <= max_samples        (m.z: the pixel's own count in the moments record)
 *                     — an unmeasured pixel is selected — and counts as rpt_noise_count does; the call stops with converged = 1 when every pixel is
 *                     measured and above <= max_above, with converged = 0 when nothing is selected, and otherwise renders batch_samples for the selected.
 *                     A pixel's record changes only when it is sampled, so a pixel at or below the threshold is never selected again, and (max_above = 0,
 *                     moments zeroed before the call) its final count has a CLOSED FORM: the first count of the schedule min_samples, min_samples +
 *                     batch_samples, ... at which its noise was at or below the threshold, else the last count of the schedule that is <= max_samples.
 *                     The passes made = the most steps any pixel took.  With max_above > 0 the call stops at the first pass before which at most that many
 *                     were above.  m.z counts from where the moments were last zeroed (rpt_set_moments, rpt_reset): call it on a fresh record.
 *                     STOPPING ON AN EMPIRICAL VARIANCE BIASES THE ESTIMATE: a pixel stops when its samples so far happen to agree, which favours
 *                     low estimates of bright, rare contributions — the limit stated above for min_samples, here per pixel.  A pixel whose first
 *                     min_samples samples were all equal stops at min_samples.
 *                     out: passes = masked passes made; min / max_pixel_samples = the range of m.z over the owned pixels; pixel_samples = what this call
 *                     rendered, uniform phase included; counts = the last count (the state at return); ms = host clock over the call.
 * rpt_multi_*         the same on every rank: each selects among its own pixels, above and selected are summed over the ranks, every rank's pass is
 *                     enqueued before any is waited for, and the image is gathered once at the end.  Round-robin tiles do not balance a noise map: the
 *                     ranks finish a pass at different times.
 * RPT_EINVAL, the context stays usable: a null mask, target or out; calls before scene, config or reset; the target refusals of rpt_render_to_noise.  A
 * context that can keep only one slot per pixel for the whole image is not refused as such: a pass's view has its own slot count. */
int rpt_render_pixels(rpt_ctx *ctx, const uint8_t *mask, uint32_t n_samples);

typedef struct rpt_adaptive_result {
    uint32_t passes, converged;            /* masked passes made; 1 = every pixel measured and at most max_above left above the threshold */
    uint32_t min_pixel_samples, max_pixel_samples;   /* of the moments' counts (m.z) over the owned pixels */
    uint64_t pixel_samples;                /* pixel-samples this call rendered, uniform phase included */
    rpt_noise_counts counts;               /* as rpt_noise_count at the end */
    double ms;
} rpt_adaptive_result;
int rpt_render_adaptive(rpt_ctx *ctx, const rpt_noise_target *target, rpt_adaptive_result *out);
int rpt_counts_uniform(rpt_ctx *ctx, uint32_t *uniform_out);
int rpt_multi_render_pixels(rpt_multi *m, const uint8_t *mask, uint32_t n_samples);
int rpt_multi_render_adaptive(rpt_multi *m, const rpt_noise_target *target, rpt_adaptive_result *out);

/* --- adaptive sampling by a pixel's NEIGHBOURHOOD (no reference equivalent) -----------------------------------------------------------------------------
 * Opt-in, a second entry point: rpt_render_adaptive, its kernels and its results are what they were.  rpt_render_adaptive stops a pixel as soon as its OWN
 * empirical noise is at or below the threshold, so a pixel whose samples so far all agree (noise_rel == 0: a dark pixel that has not met the light yet) is
 * never sampled again.  Here a pixel keeps being sampled while ANY PIXEL OF ITS WINDOW is still noisy.  With m_q the moments record of pixel q:
 *     above(q)    = !(noise_rel(m_q) <= threshold)                      (an unmeasured record, +inf and a NaN are above)
 *     fits(p)     = m_p.z + batch_samples <= max_samples
 *     near(p)     = some q with |x_q - x_p| <= radius and |y_q - y_p| <= radius, inside the image AND inside p's own RPT_TILE x RPT_TILE tile, has above(q)
 *     selected(p) = near(p) && fits(p)
 * near(p) counts p itself; fits is applied after the window, so a pixel at the cap is never selected, yet keeps its neighbours selected.  radius 0 is the
 * rule of rpt_render_adaptive and launches exactly its kernels: rpt_render_adaptive_window(ctx, target, 0, out) IS rpt_render_adaptive, bit for bit and field
 * for field except ms.  radius 1 .. RPT_ADAPTIVE_MAX_RADIUS: one kernel with a workgroup per owned tile (csrc/k_adaptive.h k_ad_window) writes the flags,
 * and the ordered compaction, the masked pass and everything stated above for them are unchanged.
 * THE WINDOW IS CLIPPED TO THE PIXEL'S TILE on purpose: a rank holds the records of its own tiles only, and with the clip the selection — and therefore the
 * image — does not depend on the partition or on the number of GPUs, as for every other call here.  The price is a SEAM: a quiet pixel on a tile edge does
 * not see a noisy neighbour across it.
 * The loop and its stop conditions are rpt_render_adaptive's: counts (pixels / measured / above) are still about each pixel's OWN noise; converged when every
 * pixel is measured and above <= max_above; done and not converged when nothing is selected; else batch_samples for the selected.  A pass that selects every
 * owned pixel — with a large radius the common case — runs as the uniform call it amounts to.
 * A pixel at or below the threshold can be selected again, so THE CLOSED FORM ABOVE HOLDS FOR RADIUS 0 ONLY; the prediction of a pixel's final count for
 * radius > 0 is a pass-by-pass simulation (tests/adaptive_window_ref.py), which tests/test_gpu_adaptive_window.py holds the device to, word for word.
 * WHAT THE RULE STILL CANNOT SEE: a whole region (its windows as clipped) in which no pixel has met the light yet — all of it looks converged.  min_samples
 * stays the answer there, and the bias of stopping on an empirical variance is reduced, not removed.
 *
 * rpt_adaptive_mask     the pixels the NEXT pass of that call would render: width*height bytes, row-major, 1 = selected, other ranks' pixels 0; counts_out
 *                     (nullable) as rpt_noise_count.  Renders nothing, changes nothing; synchronises.  rpt_render_pixels(ctx, that mask, batch_samples)
 *                     equals one pass, so a host can drive or draw the sampling map itself.  RPT_EINVAL while moments are off.
 * rpt_multi_*           as rpt_multi_render_adaptive; rpt_multi_adaptive_mask sums the counts over the ranks and merges their masks on the host.
 * RPT_EINVAL, the context stays usable: everything rpt_render_adaptive refuses, radius > RPT_ADAPTIVE_MAX_RADIUS, a null mask_out. */
#define RPT_ADAPTIVE_MAX_RADIUS 8
int rpt_render_adaptive_window(rpt_ctx *ctx, const rpt_noise_target *target, uint32_t radius, rpt_adaptive_result *out);
int rpt_multi_render_adaptive_window(rpt_multi *m, const rpt_noise_target *target, uint32_t radius, rpt_adaptive_result *out);
int rpt_adaptive_mask(rpt_ctx *ctx, const rpt_noise_target *target, uint32_t radius, uint8_t *mask_out, rpt_noise_counts *counts_out);
int rpt_multi_adaptive_mask(rpt_multi *m, const rpt_noise_target *target, uint32_t radius, uint8_t *mask_out, rpt_noise_counts *counts_out);

/* --- scene preparation on the device ---------------------- */
/* BVHBuilder::new(vertices, indices).sah_samples(n).build()  (reference src/bvh.rs:59-324, the call at
 * src/asset.rs:196) on the GPU: reorders `triangles` in place and writes the node pool exactly as the sequential
 * builder does (same nodes, same order, same bits; tests/test_gpu_bvh_build.py).  Host pointers, no context needed;
 * vertices are Vec4 (xyzw) as in bvh.rs:52; nodes_capacity >= 2 * n_triangles - 1; sah_samples <= 128.
 * device_ms_out (nullable) receives the device time of the build proper.  Errors: rpt_last_error(NULL). */
int rpt_bvh_build_gpu(int device_id, const float *vertices_xyzw, size_t n_vertices, rpt_triangle *triangles,
                      size_t n_triangles, uint32_t sah_samples, rpt_bvh_node *nodes_out, size_t nodes_capacity,
                      size_t *n_nodes_out, double *device_ms_out);

/* build_light_pick_table(vertices, indices, compute_emissive_mask(..), materials)  (reference src/light_pick.rs:13-122, the call at
 * src/asset.rs:197-198) with its parallel parts on the GPU — Heron areas and powers, probabilities, the stable sort, the table — and the
 * three order-dependent f32 chains (the two sums of :39-64 in index order, the robin-hood fill of :89-104) on the host between the device passes
 * (csrc/rpt_lights.hip: a question of latency per dependent operation, measured).  Same entries, same order, same bits as the sequential builder (tests/test_gpu_light_table.py).  Host pointers, no
 * context; entries_capacity >= the number of emissive triangles (>= 1: a scene without lights yields the one-entry sentinel, ratio = -1).
 * ms_out (nullable): 4 doubles — total, device passes, host chains, transfers.  A NaN pick probability — a NaN vertex, a total power of 0 (every emissive
 * triangle degenerate) or inf — is refused by name (RPT_ESCENE): the reference's answer there depends on its sequential sort, which rpt_light_table_build restates. */
int rpt_light_table_build_gpu(int device_id, const float *vertices_xyzw, size_t n_vertices, const rpt_triangle *triangles, size_t n_triangles,
                              const rpt_material_data *materials, size_t n_materials, rpt_light_pick_entry *entries_out, size_t entries_capacity,
                              size_t *n_entries_out, uint32_t *n_emissive_out, double *ms_out);

/* (The test hooks — rpt_debug_*: device math against the host build, ray parity through the production kernels, the order probes' host driver — are
 * declared in rpt/rpt_debug.h: exported by the same library, no part of the boundary a host binds.) */

#ifdef __cplusplus
}
#endif
#endif /* RPT_H */
