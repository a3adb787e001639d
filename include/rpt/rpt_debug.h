/*
 * rpt_debug.h — test hooks of librpt_hip.so.  NOT part of the drop-in boundary (include/rpt/rpt.h is what replaces the gpgpu-rs calls of
 * src/trace.rs:136-224); nothing here is needed by, or bound in, a host (ffi/rpt.rs).  They exist so that the tests can hold single pieces of the device
 * code — the shared math, the traversal kernels, the order probes, the gather's point-to-point calls — against the CPU oracle piece by piece.
 */
#ifndef RPT_DEBUG_H
#define RPT_DEBUG_H

#include "rpt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Evaluate one shared-math function on the DEVICE over n floats so tests can
 * check bit-equality with the host build of the same header. op: 0 sin, 1 cos,
 * 2 acos, 3 exp, 4 pow(x,y), 5 asin, 6 atan2(y=x_in, x=y_in), 7 sqrt, 8 IEEE x/y,
 * 9 x/y through the traversal's guarded exact fast-division path (rpt_fastdiv.h), 10 the sky march's float-only exp
 * (rpt_math.h exp_sky), 11 an atlas texel channel u8 / 255 (rpt_math.h unorm8); the helpers of rpt_math.h: 12 fminr(x, y),
 * 13 fmaxr(x, y), 14 floorr, 15 ceilr, 16 f2u32_sat(x) returned as the word's bits, 17 atanr, 18 powi5, 19 absr; the double a
 * building block returns, as the bits of its low (even op) and high (odd op) word: 20/21 sin_poly and 22/23 cos_poly on [-1, 1],
 * 24/25 exp_core on [-700, 700], 26/27 log_core on the positive finite floats, 28/29 asin_poly(x, x^2) on [-1, 1], 30/31 atan01 on
 * [0, 1] (0 outside these domains).  Every other op is refused (RPT_EINVAL). */
int rpt_debug_math(rpt_ctx *ctx, int op, const float *x, const float *y, float *out, size_t n);
/* Same on the HOST build (no device needed, ctx may be NULL). */
int rpt_debug_math_host(int op, const float *x, const float *y, float *out, size_t n);
/* The decision rpt_upload_scene takes about the shadow walks' visiting order (rpt_shadow_order), without a device: the sequential driver of the probe
 * (shadow_order.h) — the checker of the kernels rpt_upload_scene runs.
 * flip_out (nullable): per child pair p = nodes (2p + 1, 2p + 2), 1 where the fixed order enters the right child first. */
int rpt_debug_shadow_order_host(const rpt_per_vertex_data *vertices, size_t n_vertices, const rpt_triangle *indices, size_t n_triangles,
                                const rpt_bvh_node *nodes, size_t n_nodes, const rpt_material_data *materials, size_t n_materials,
                                const rpt_light_pick_entry *light_pick, size_t n_light_pick, uint32_t *fixed_out, double *visits_near_out,
                                double *visits_fixed_out, uint32_t *probe_rays_out, uint8_t *flip_out);
/* The reason behind that decision, in the probe's own words ("node pool is not pair-shaped", "no lights", "no probe ray could be formed",
 * "RPT_SHADOW_ORDER=fixed", ...): of the scene the context holds, or with ctx NULL of this thread's last rpt_debug_shadow_order_host call.  A static
 * string, never NULL ("" for a context without a scene, and before the first host call). */
const char *rpt_debug_shadow_order_why(rpt_ctx *ctx);
/* The same for the order of the hit-or-miss lanes of the last extension rays (rpt_last_bounce_order): rule_out 0 near child first, 1 / 2 / 3 the fixed rules. */
int rpt_debug_last_order_host(const rpt_per_vertex_data *vertices, size_t n_vertices, const rpt_triangle *indices, size_t n_triangles,
                              const rpt_bvh_node *nodes, size_t n_nodes, const rpt_material_data *materials, size_t n_materials,
                              uint32_t *rule_out, double *visits_out /* [4] */, uint32_t *probe_rays_out, uint8_t *flip_out);
/* Exhaustive device-side check of a cheap exact operation of rpt_math.h against its IEEE form over the float bit patterns
 * [lo_bits, lo_bits + count): op 0 sqrtr vs the correctly rounded sqrtf, op 1 div_const_nontiny(x, y, RN(1/y)) vs x / y, op 2 the one-instruction
 * f32 -> i32 conversion vs Rust's `as i32` written out.  Returns the
 * number of arguments whose results differ in any bit (NaN == NaN) and the smallest such bit pattern (0xffffffff if none). */
int rpt_debug_math_sweep(rpt_ctx *ctx, int op, uint32_t lo_bits, uint64_t count, float y, uint64_t *mismatches_out,
                         uint32_t *first_bad_bits_out);
/* rptm::rcp_rn (csrc/rpt_rcp.h: the reciprocal from v_rcp_f32 and one residual step, the division outside its guard; window != 0: rcp_rn_window, the step alone, for arguments inside the window) on the device: over n floats, and
 * compared on the device with the compiler's `1.0f / x` over the bit patterns [lo_bits, lo_bits + count), count <= 2^32 — the number of arguments whose
 * results differ in any bit (NaNs too: word for word) and up to 64 of those bit patterns (0xffffffff in the unused places of bad_bits_out[64]). */
int rpt_debug_rcp(rpt_ctx *ctx, int window, const float *x, float *out, size_t n);
int rpt_debug_rcp_sweep(rpt_ctx *ctx, int window, uint32_t lo_bits, uint64_t count, uint64_t *mismatches_out, uint32_t *bad_bits_out);
/* Trace n rays through the uploaded BVH on the device. any_hit = 0: nearest
 * (kernels/src/intersection.rs:169-171) ; 1: any-hit with max_t
 * (:173-175) ; 2: the segment-bounded any-hit walk of RPT_SHADOW_SEGMENT (rpt.h
 * rpt_set_shadow_mode: a child box is entered only if also tmin <= max_t), through the
 * same one-ray-per-lane kernel, .hit is what it answers.  Outputs per ray: t, triangle_index, flags (bit0 hit, bit1 backface). */
int rpt_debug_trace_rays(rpt_ctx *ctx, int any_hit, size_t n,
                         const float *origins_xyz, const float *dirs_xyz, const float *max_t,
                         float *out_t, uint32_t *out_tri, uint32_t *out_flags);
/* Nearest hits of n rays through the PRODUCTION traversal stage — the kernel and grid an iteration of rpt_render uses for the
 * context's scene and state (persistent LDS stream, streamed global-memory walk, ... per scene and developer knobs), fed through
 * the context's own slots; same outputs as rpt_debug_trace_rays(any_hit = 0).  Needs a configuration with at least n slots;
 * afterwards the context is as after rpt_reset with nothing rendered (call rpt_reset before rendering again). */
int rpt_debug_trace_rays_production(rpt_ctx *ctx, size_t n, const float *origins_xyz, const float *dirs_xyz,
                                    float *out_t, uint32_t *out_tri, uint32_t *out_flags);
/* n caller-chosen rays through ANY of the walks rpt_render launches: the hook writes the rays where the pipeline keeps them (the context's slots, or its
 * sharded shadow queue) and calls rpt_launch_nearest / rpt_launch_shadow exactly as an iteration of rpt_render does — it chooses no kernel, span, grid or
 * LDS size, so the scene, rpt_set_shadow_mode and the developer knobs (RPT_NO_LDS_SCENE, RPT_COOP_LEAVES, RPT_STACK_BITS, RPT_SHADOW_ORDER, RPT_LAST_ORDER,
 * RPT_SLOT_Q_SHIFT) select the instantiation as they do in a render.  kind:
 *   RPT_WALK_NEAREST_PLAIN  what rpt_debug_trace_rays_production does (that call is this kind).
 *   RPT_WALK_NEAREST_FIRST  the launch of a render call's first iteration: the streamed LDS walk stages its planes with ONE origin subtracted, so EVERY
 *                           origin must equal the configuration's cam_position bit for bit (else RPT_EINVAL).  The slots are prepared as k_generate_first
 *                           leaves them; the form in which the walk starts the paths itself stays covered by renders only.
 *   RPT_WALK_NEAREST_LAST   the launch of the last extension rays of a batch of known length without NEE, in the form that writes hit records (one slot per
 *                           pixel): a ray that passes the test of no emissive triangle may stop at its first accepted triangle, so its record names A
 *                           triangle it hits, not the nearest.  The path-ending form (several slots per pixel: the walk adds emission, parks misses and
 *                           writes HIT_DONE itself) stays covered by renders only.
 *   RPT_WALK_SHADOW         any-hit rays (max_t required) through the shadow queue, whose shards the hook fills UNEVENLY so that the swept positions
 *                           include unfilled ones, then rpt_launch_shadow (k_shadow_resolve behind the streamed LDS walk).  Entry i carries the
 *                           contribution (1, 1 + i % 4093, 0) for slot i: out_flags bit 0 = occluded (the slot's radiance stayed 0); a radiance record
 *                           that is neither is an entry resolved into the wrong slot or twice — RPT_EHIP, the message names the ray.  out_t and out_tri
 *                           are left zero: the production kernels keep no record.
 * Outputs of the nearest kinds as rpt_debug_trace_rays(any_hit = 0).  n == 0: RPT_OK, nothing launched.  RPT_EINVAL: no scene or configuration, n above
 * the slot count (SHADOW: or more than the uneven fill leaves room for in the queue), SHADOW without max_t.  Afterwards the context is as after
 * rpt_reset with nothing rendered, its counters apart: CALL rpt_reset BEFORE RENDERING AGAIN. */
#define RPT_WALK_NEAREST_PLAIN 0
#define RPT_WALK_NEAREST_FIRST 1
#define RPT_WALK_NEAREST_LAST 2
#define RPT_WALK_SHADOW 3
int rpt_debug_walk_production(rpt_ctx *ctx, int kind, size_t n, const float *origins_xyz, const float *dirs_xyz, const float *max_t /* shadow kinds only */,
                              float *out_t, uint32_t *out_tri, uint32_t *out_flags);

/* The two BSDFs of the reference's kernels crate that trace_pixel never instantiates (kernels/src/bsdf.rs:46-176,
 * SURVEY.md 8f N4), evaluated on the device.  One item = 16 floats in: view(3) normal(3) r(3) albedo(3) ior roughness
 * pad(2); 8 floats out: pdf, lobe (u32 bits), spectrum(3), direction(3).  kind 0 Lambertian::sample, 1 Glass::sample,
 * 2 Lambertian::{evaluate, pdf} (sample_direction = r), 3 Glass::{evaluate, pdf} (lobe = (u32) r.x). */
int rpt_debug_bsdf(rpt_ctx *ctx, int kind, size_t n, const float *in, float *out);
/* The image sampler of the shade stage, the sky stage and the denoiser's guides (csrc/k_shade.h sample_by_lod: the CPU polyfill's bilinear, wrapping lookup,
 * shared_structs/src/image_polyfill.rs:32-55) on an image of the hook's own, one coordinate per thread: texels are width * height RGBA8 words (is_u8 != 0:
 * an atlas, texel = (r, g, b, 255) / 255) or width * height float Vec4s (a skybox), within the sizes rpt_upload_scene accepts; coords_uv 2 floats and
 * out_rgba 4 floats per coordinate.  Needs no scene and leaves the context as it was. */
int rpt_debug_sample_image(rpt_ctx *ctx, int is_u8, const void *texels, uint32_t width, uint32_t height, size_t n, const float *coords_uv, float *out_rgba);
/* The gather's point-to-point calls against the collective library the process resolved (rpt_comm_library), without a second GPU:
 * inside one ncclGroupStart / ncclGroupEnd this rank posts ncclRecv from rank - 1 and ncclSend to rank + 1 (one rank: to and from
 * itself) on the communicator's second stream, ordered by the same events as rpt_gather_async; n_floats of a known pattern travel
 * as ncclFloat and are compared on the host.  Needs rpt_comm_init; collective (every rank calls it). */
int rpt_debug_comm_selftest(rpt_ctx *ctx, uint32_t n_floats, uint64_t *mismatches_out);

/* The denoise filter of rpt_denoise on the HOST: the same header (csrc/k_denoise.h) in a plain loop over the pixels — no device needed, as rpt_debug_math_host.
 * mean_rgb, albedo, normal, position: width*height*3 floats; depth: width*height floats; kind: width*height words (the layouts of rpt_read_guides); params
 * NULL = defaults; out_rgb: width*height*3 floats.  RPT_EINVAL for the parameter values rpt_denoise refuses. */
int rpt_debug_denoise_host(uint32_t width, uint32_t height, const float *mean_rgb, const float *albedo, const float *normal, const float *position,
                           const float *depth, const uint32_t *kind, const rpt_denoise_params *params, uint32_t tonemap_op, float *out_rgb);

/* The variance-guided filter of rpt_denoise_variance on the HOST: the same headers (csrc/k_denoise.h, k_moments.h) in a plain loop — no device needed.  The
 * planes of rpt_debug_denoise_host and moments_xyzw: width*height records of 4 floats (what rpt_read_moments returns); params NULL = defaults; out_rgb:
 * width*height*3 floats; out_variance (nullable): width*height floats, unknown = +inf.  RPT_EINVAL for the parameter values rpt_denoise_variance refuses. */
int rpt_debug_denoise_variance_host(uint32_t width, uint32_t height, const float *mean_rgb, const float *albedo, const float *normal, const float *position,
                                    const float *depth, const uint32_t *kind, const float *moments_xyzw, const rpt_denoise_var_params *params, uint32_t tonemap_op,
                                    float *out_rgb, float *out_variance);

/* rpt_denoise_temporal on the HOST: the same headers (csrc/k_temporal.h, k_denoise.h) in a plain loop — no device needed.  The current view's planes and
 * moments as rpt_debug_denoise_variance_host takes them; camera: the current view (position, rotation, width and height are read); prev_camera NULL = no
 * history, else the previous view's camera, its guide planes prev_normal, prev_position, prev_kind and its history records prev_history: width*height
 * records of 6 floats (e_h.r, e_h.g, e_h.b, N, mu1, mu2).  params NULL = defaults.  out_variance, out_history (T per pixel), out_records (the new history,
 * 6 floats per pixel) and pixels_with_history_out are nullable.  RPT_EINVAL for the parameter values rpt_denoise_temporal refuses and for a camera whose
 * width or height is not the image's. */
int rpt_debug_denoise_temporal_host(uint32_t width, uint32_t height, const float *mean_rgb, const float *albedo, const float *normal, const float *position,
                                    const float *depth, const uint32_t *kind, const float *moments_xyzw, const rpt_tracing_config *camera,
                                    const rpt_tracing_config *prev_camera, const float *prev_normal, const float *prev_position, const uint32_t *prev_kind,
                                    const float *prev_history, const rpt_temporal_params *params, uint32_t tonemap_op, float *out_rgb, float *out_variance,
                                    float *out_history, float *out_records, uint64_t *pixels_with_history_out);

/* The firefly clamp of rpt_denoise_variance / rpt_denoise_temporal on the HOST: the same header (csrc/k_firefly.h ff_pixel) in a plain loop — no device needed.
 * mean_rgb (the mean in radiance units, before any demodulation) and albedo: width*height*3 floats; kind: width*height words; moments_xyzw: width*height
 * records of 4 floats; counts (nullable): width*height floats, the count every pixel's mean was divided by — NULL: every pixel has (float)samples; the three
 * clamp parameters of rpt_denoise_var_params; demodulated: what the call would decide (base.iterations != 0 && base.demodulate != 0).  out_rgb: c',
 * width*height*3 floats; out_moments_xyzw: m', width*height records; out_mask: width*height bytes, 1 = clamped (an unclamped pixel's c and m are copied).
 * Every output is nullable.  RPT_EINVAL for the parameter values rpt_denoise_variance refuses; clamp_scale == 0 copies the inputs.
 * rpt_debug_denoise_variance_host and rpt_debug_denoise_temporal_host honour the clamp fields too; they are handed no count and take count_p = m_p.z. */
int rpt_debug_firefly_host(uint32_t width, uint32_t height, const float *mean_rgb, const float *albedo, const uint32_t *kind, const float *moments_xyzw,
                           const float *counts, uint32_t samples, float clamp_scale, float clamp_floor, uint32_t clamp_radius, uint32_t demodulated,
                           float *out_rgb, float *out_moments_xyzw, uint8_t *out_mask);

/* One step of the chain of rpt_set_guides_through_glass on the HOST: the same header (csrc/k_guides_glass.h dn_glass_step) in a plain loop over n rays — no
 * device needed, so a test can drive whole chains with any nearest-hit walk (the oracle's).  The scene as rpt_upload_scene takes it, without the tree and the
 * lights; models: one record per material, or NULL for "every material is PBR"; max_interfaces 0..8.  Per ray: origins_xyz, dirs_xyz (3 floats; overwritten
 * with the next ray where the chain goes on), its nearest hit as rpt_debug_trace_rays reports it, and the chain so far — chain_albedo (A, 3 floats; a fresh
 * chain: 1, 1, 1), chain_length (L; 0), chain_interfaces (m; 0) — all three updated in place (a final chain's chain_length is the guide's depth).
 * active_out: 1 = the chain goes on into the next round; else kind_out, normal_out, albedo_out (A * a) hold the final records and exhausted_out says whether
 * it ended on a glass surface.  position = primary origin + primary direction * chain_length is the caller's.  RPT_EINVAL for null pointers, a triangle, vertex
 * or material index out of range, max_interfaces above 8, a texture flag without an atlas. */
int rpt_debug_glass_step_host(const rpt_per_vertex_data *vertices, size_t n_vertices, const rpt_triangle *indices, size_t n_triangles,
                              const rpt_material_data *materials, size_t n_materials, const uint8_t *atlas_rgba8, uint32_t atlas_w, uint32_t atlas_h,
                              const rpt_material_model *models, uint32_t max_interfaces, size_t n, float *origins_xyz, float *dirs_xyz, const float *hit_t,
                              const uint32_t *hit_tri, const uint32_t *hit_flags, float *chain_albedo, float *chain_length, uint32_t *chain_interfaces,
                              uint8_t *active_out, uint32_t *kind_out, float *normal_out, float *albedo_out, uint8_t *exhausted_out);

/* noise_rel and the counts of rpt_noise_count on the HOST: the same header (csrc/k_moments.h) in a plain loop over n moments records (4 floats each: sum Y,
 * sum Y^2, n, max Y) — no device needed.  rel_out (n floats) and counts_out are nullable; counts_out->pixels = n.  RPT_EINVAL for a negative or NaN threshold. */
int rpt_debug_noise_host(const float *moments_xyzw, size_t n, float threshold, float *rel_out, rpt_noise_counts *counts_out);

/* The selection rule of rpt_render_adaptive and the ordered compaction of a masked pass on the HOST: the same header (csrc/k_adaptive.h) in a plain loop
 * over n moments records — no device needed.  flags_out (n bytes: 1 = selected), active_out (room for n indices: the selected records' indices, ascending)
 * and n_active_out are nullable.  RPT_EINVAL for a negative or NaN threshold. */
int rpt_debug_adaptive_select_host(const float *moments_xyzw, size_t n, float threshold, uint32_t batch_samples, uint32_t max_samples, uint8_t *flags_out,
                                   uint32_t *active_out, size_t *n_active_out);

/* The window rule of rpt_render_adaptive_window on the HOST: the same header (csrc/k_adaptive.h: ad_above, ad_dilate_row, ad_dilate_rows, ad_fits) in a plain
 * loop over every RPT_TILE x RPT_TILE tile of a row-major image of width*height moments records — no device needed.  flags_out: width*height bytes, 1 =
 * selected.  RPT_EINVAL for a null pointer, a width or height outside 1..65535, a negative or NaN threshold and a radius above RPT_ADAPTIVE_MAX_RADIUS. */
int rpt_debug_adaptive_window_host(const float *moments_xyzw, uint32_t width, uint32_t height, float threshold, uint32_t batch_samples, uint32_t max_samples,
                                   uint32_t radius, uint8_t *flags_out);

/* Measuring aid (tools/adaptive_probe.py --gpu-window): the device time of the selection step of rpt_render_adaptive_window alone — HIP events on the context's
 * stream around the select kernels of one pass, `repeats` times, after one untimed round; ms_out: `repeats` floats.  Renders nothing, the selection is dropped.
 * Refuses what rpt_adaptive_mask refuses, a null ms_out and repeats == 0. */
int rpt_debug_adaptive_select_ms(rpt_ctx *ctx, const rpt_noise_target *target, uint32_t radius, uint32_t repeats, float *ms_out);

/* The gather's second wire format (rpt_gather_set_moments; csrc/k_gather.h) on the HOST — no device needed.
 * rpt_debug_gather_layout: for an image of width x height over `world` ranks, stride_pixels_out = the largest block of any rank; slot_floats_out = floats of
 * one rank's slot (with_moments: 2 * stride * 4 + 4, else stride * 4); block_pixels_out[world] = every rank's own pixels; message_floats_out[world] = the
 * count of its one ncclSend (with_moments: the whole slot for every rank; else its block, 0 = the rank posts nothing).  Every output is nullable.
 * rpt_debug_gather_host: the host build of pack -> slots -> un-tile.  accum_blocks, moments_blocks: the ranks' tile-major blocks one behind the other
 * (width*height records of 4 floats in all); trailers: 4 words per rank as a rank would write them — RPT_GATHER_FORMAT, counts_nonuniform, the uniform
 * sample count, the rank's pixel count.  slots_io (nullable; world * slot floats): the landing buffer, as the caller initialised it — the padding behind
 * a block is never written — else a zeroed one of the hook's own; image_out, moments_out (nullable): width*height records, row-major; info_out (nullable):
 * the words of rpt_gathered_info_get.  RPT_EINVAL for a width or height outside 1..65535, a world outside 1..64, null inputs. */
#define RPT_GATHER_FORMAT 0x52504d32u
int rpt_debug_gather_layout(uint32_t width, uint32_t height, uint32_t world, uint32_t with_moments, uint64_t *stride_pixels_out, uint64_t *slot_floats_out,
                            uint64_t *block_pixels_out, uint64_t *message_floats_out);
int rpt_debug_gather_host(uint32_t width, uint32_t height, uint32_t world, const float *accum_blocks, const float *moments_blocks, const uint32_t *trailers,
                          float *slots_io, float *image_out, float *moments_out, rpt_gathered_info *info_out);

/* Test aid: the next asynchronous batches of this context enqueue one iteration too few — proves that the completion checks (rpt_wait, the next
 * batch's k_generate_first) notice a sample left in flight instead of losing it. */
int rpt_debug_short_batch(rpt_ctx *ctx, int on);

/* Test aid: on != 0 makes the render calls of this context launch the models variant of the shade stage (rpt_set_material_models) whatever the records
 * say — on an all-PBR scene it must give the plain kernels' image and counters bit for bit. */
int rpt_debug_force_model_kernels(rpt_ctx *ctx, int on);

/* Test aid: on != 0 makes the render calls of this context launch the volumes variant of the shade stage (rpt_set_material_volumes) whatever the records
 * say — with no records, or with all-zero ones, it must give the models variant's image and counters bit for bit.
 * rpt_debug_last_shade_variant: which build of the shade stage the context's last shade launch was — 0 k_shade, 1 k_shade_models, 2 k_shade_volumes,
 * 3 k_shade_punctual. */
int rpt_debug_force_volume_kernels(rpt_ctx *ctx, int on);
int rpt_debug_last_shade_variant(rpt_ctx *ctx, uint32_t *variant_out);

/* The arithmetic of rpt_set_material_volumes alone (csrc/k_volume.h vol_transmit) on n items: throughput_xyz, sigma_xyz, out_xyz 3 floats per item, t one.
 * on_device == 0: the host build of the header — no device needed, ctx may be NULL; else the same header through a device kernel of the context's device.
 * RPT_EINVAL for null pointers (and a null ctx with on_device != 0). */
int rpt_debug_volume_transmit(rpt_ctx *ctx, int on_device, const float *throughput_xyz, const float *sigma_xyz, const float *t, size_t n, float *out_xyz);

/* The camera rays of rpt_set_camera_lens (csrc/k_lens.h lens_ray) for n chosen (pixel, key) pairs: pixels_xy[i] = x | y << 16, keys[i] = the sample's LDS key
 * n + offset; origins_out, dirs_out: 3 floats per pair.  config: position, rotation, width and height are read; lens NULL = the default.
 * rpt_debug_lens_rays_host: the host build of the header — no device needed.  rpt_debug_lens_rays: the same header through a device kernel, with the
 * configuration and the lens the CONTEXT holds.  RPT_EINVAL for null pointers, a lens rpt_set_camera_lens refuses, a width or height of 0. */
int rpt_debug_lens_rays_host(const rpt_tracing_config *config, const rpt_camera_lens *lens, const uint32_t *pixels_xy, const uint32_t *keys, size_t n,
                             float *origins_out, float *dirs_out);
int rpt_debug_lens_rays(rpt_ctx *ctx, const uint32_t *pixels_xy, const uint32_t *keys, size_t n, float *origins_out, float *dirs_out);

/* Test aid: on != 0 makes the render calls of this context launch the punctual variant of the shade stage (rpt_set_punctual_lights) under NEE modes 1 and 2
 * whatever the lights say — with no lights it must give the other variants' image and counters bit for bit.  nee = 0 keeps the other variants.
 * rpt_debug_last_shade_variant then reports 3 (k_shade_punctual). */
int rpt_debug_force_punctual_kernels(rpt_ctx *ctx, int on);

/* The arithmetic of rpt_set_punctual_lights alone (csrc/k_punctual.h punctual_sample) on n_items items against n_lights host records and a share q: hits_xyz 3
 * floats per item, l1 one; out per item: j_out one word, dirs_out (L) 3 floats, max_t_out one, e_out (E) 3 floats, pick_pdf_out one.  The records are
 * converted as the setter converts them.  rpt_debug_punctual_sample_host: the host build of the header — no device needed.  rpt_debug_punctual_sample: the
 * same header through a device kernel of the context's device.  RPT_EINVAL for null pointers, n_lights == 0, a q outside (0, 1] and records that
 * rpt_set_punctual_lights refuses (the hooks and the setter share one check).
 * rpt_debug_punctual_lights_check: that check alone, no context and no device needed — everything the setter refuses except a call before a scene;
 * scene_has_emitters stands for the scene (non-zero: the light table is not the sentinel, so pick_share must lie in (0, 1)); message_out (nullable,
 * capacity bytes, zero-terminated) receives the message the setter would leave in the context.  RPT_OK or RPT_EINVAL. */
int rpt_debug_punctual_lights_check(const rpt_punctual_light *lights, size_t n, float pick_share, int scene_has_emitters, char *message_out, size_t capacity);
int rpt_debug_punctual_sample_host(const rpt_punctual_light *lights, size_t n_lights, float q, const float *hits_xyz, const float *l1, size_t n_items,
                                   uint32_t *j_out, float *dirs_out, float *max_t_out, float *e_out, float *pick_pdf_out);
int rpt_debug_punctual_sample(rpt_ctx *ctx, const rpt_punctual_light *lights, size_t n_lights, float q, const float *hits_xyz, const float *l1, size_t n_items,
                              uint32_t *j_out, float *dirs_out, float *max_t_out, float *e_out, float *pick_pdf_out);

#ifdef __cplusplus
}
#endif
#endif /* RPT_DEBUG_H */
