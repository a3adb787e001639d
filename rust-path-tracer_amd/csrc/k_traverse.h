/*
 * k_traverse.h — BVH traversal + ray/triangle intersection stage.
 *
 * Produces, per ray, exactly what the reference's stack traversal produces
 * (kernels/src/intersection.rs:177-234, with intersect_aabb :104-122 and
 * muller_trumbore :9-54): same visiting order, same strict comparisons, same
 * f32 operations — so t / triangle index / backface are bit-identical to the
 * CPU path.  What differs is the machinery:
 *   - one wave64 lane per ray, rays read as two coalesced float4 records;
 *   - the traversal stack lives in LDS, laid out [entry][lane] so that every
 *     ds_read/ds_write of a wave is bank-conflict free regardless of the
 *     per-lane stack depth (lane l always hits bank l mod 32 of its half);
 *   - the near child is entered directly (the reference pushes it and pops it
 *     straight back, :229 then :183), only the far child is pushed;
 *   - both children of an inner node are adjacent (right = left + 1), so one
 *     node visit is 4 float4 loads = 64 contiguous bytes;
 *   - leaf triangles come from a pre-gathered (a, b-a, c-a) array instead of
 *     index buffer -> 3 x 64-byte vertex records (same f32 subtractions, done
 *     once at upload).
 * Traversal order is part of the NEAREST-hit result (ties in t keep the first
 * triangle visited): no reordering there.  The ANY-hit walk (light_pick.rs:141-148
 * + intersection.rs:173-234 with NEAREST_HIT = false) must match the reference in
 * `.hit` ONLY — light_pick.rs:148 reads nothing else: result.t stays 1e6 until the
 * first accept, which returns (:191-203), boxes are pruned against that constant
 * (:212-213: no "max_t" box pruning in the exact walk; the opt-in SEGMENT walks, shadow_segment_bound below, add it), so the set of boxes a ray may enter and with
 * it `.hit` are independent of the order siblings are visited in.  FIXED = true
 * walks a copy of the tree whose pairs were flipped at upload (shadow_order.h: the
 * preferred child in the left slot) left-first: no `tl > tr`, no swap.
 *
 * The text is split by concern — k_walk.h (one ray), k_walk_stream.h (around a streamed walk), k_traverse_nearest.h, k_traverse_shadow_kernels.h — under this umbrella.
 * These kernels are sensitive to their schedule: a change of their text is checked with tools/kernel_isa_diff.py against the parent's build.
 */
#ifndef RPT_K_TRAVERSE_H
#define RPT_K_TRAVERSE_H

#include "k_common.h"
#include "k_path.h"
#include "k_walk.h"
#include "k_walk_stream.h"
#include "k_traverse_nearest.h"

/* what k_traverse_shadow does with the result of one shadow ray (light_pick.rs:148 + lib.rs:164) */
__device__ __forceinline__ void shadow_resolve(const DevState &st, const DevQueues &q, const DevConfig &cfg, uint32_t entry, uint32_t tag,
                                               bool visible) {
    const uint32_t slot = tag & 0x7fffffffu;
    const bool finish = (tag >> 31) != 0u;
    if (visible || finish) {
        float4 r4 = st.rad[slot];
        F3 radiance = f3(r4.x, r4.y, r4.z);
        if (visible) {
            float4 c = q.sh_c[entry];
            radiance = radiance + mask_nan3(f3(c.x, c.y, c.z));
        }
        if (finish) {
            finish_in_side_stage(st, cfg, slot, radiance, __float_as_uint(r4.w));
        } else {
            r4.x = radiance.x; r4.y = radiance.y; r4.z = radiance.z;
            st.rad[slot] = r4;
        }
    }
}

/* second half of the streamed LDS shadow stage: one dense pass over the shadow queue */
__global__ __launch_bounds__(RPT_BLOCK) void k_shadow_resolve(DevState st, DevQueues q, DevConfig cfg) {
    if (q.count[Q_DRAINED] != 0u) return;
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    uint32_t positions, n;
    q_extent(q.shadow_cnt, positions, n);
    if (i >= positions || !q_filled(q.shadow_cnt, i)) return;
    shadow_resolve(st, q, cfg, i, __float_as_uint(q.sh_d[i].w), q.sh_c[i].w == 0.0f);
}

/* the shadow kernels and the test hook: the exact walk under the kernels' own names, then their segment-bounded `_seg` twins (see the file's header) */
#define RPT_SHADOW_KERNEL(name) name
#define RPT_SHADOW_KERNEL_SEGMENT false
#include "k_traverse_shadow_kernels.h"
#undef RPT_SHADOW_KERNEL
#undef RPT_SHADOW_KERNEL_SEGMENT
#define RPT_SHADOW_KERNEL(name) name##_seg
#define RPT_SHADOW_KERNEL_SEGMENT true
#include "k_traverse_shadow_kernels.h"
#undef RPT_SHADOW_KERNEL
#undef RPT_SHADOW_KERNEL_SEGMENT

#endif /* RPT_K_TRAVERSE_H */
