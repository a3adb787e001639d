/*
 * k_gather.h — the second wire format of the gather (rpt_gather_set_moments, rpt_comm.hip): a rank's slot carries its accumulator block, its moments
 * record and a trailer of four words, so that rank 0 gets the whole image's moments and every rank's count state with the one collective it runs anyway.
 *
 *   slot of a rank, in float4:   [accum: stride][moments: stride][trailer: 1]          stride = the largest block of any rank (as in the plain format)
 *   trailer, four 32-bit words:  RPT_GATHER_FORMAT, counts_nonuniform, the context's uniform sample count, n_pixels
 *
 * Every slot has the same length and every half starts at a fixed offset: the root's un-tile needs no per-rank table, and a rank's message length is a
 * function of (width, height, world, setting) alone.  The padding behind a block (a rank has at most one tile fewer than the largest, and clipped ones) is zeroed when the buffers are sized and is
 * never written afterwards.  The layout arithmetic (gather_layout), the trailer's encode / decode / reduce (gather_trailer, gather_fold) and the two kernels
 * are here; rpt_debug_gather_layout / rpt_debug_gather_host (rpt_debug.hip) are the host build of the same functions.
 */
#ifndef RPT_K_GATHER_H
#define RPT_K_GATHER_H

#include "rpt_ctx.h"

/* RPT_GATHER_FORMAT (rpt_debug.h, so that the host hook's callers can write a trailer): "RPM2" — the slot carries moments and a trailer */

/* where things are in a slot, in float4 (with_moments == 0: the plain format — a slot is the padded accumulator block and nothing else) */
struct GatherLayout {
    uint64_t stride, slot, moments_at, trailer_at;
};
RPT_HD GatherLayout gather_layout(uint64_t stride, uint32_t with_moments) {
    GatherLayout l;
    l.stride = stride;
    l.slot = with_moments ? 2u * stride + 1u : stride;
    l.moments_at = stride;
    l.trailer_at = 2u * stride;
    return l;
}
/* float4 a rank of `n_pixels` sends (the root: keeps) per gather: its whole slot, or — plain — its block alone (0: the rank posts nothing) */
RPT_HD uint64_t gather_message(const GatherLayout &l, uint64_t n_pixels, uint32_t with_moments) { return with_moments ? l.slot : n_pixels; }

RPT_HD uint4 gather_trailer(uint32_t counts_nonuniform, uint32_t samples, uint32_t n_pixels) {
    return make_uint4(RPT_GATHER_FORMAT, counts_nonuniform ? 1u : 0u, samples, n_pixels);
}
/* the words of rpt_gathered_info before any trailer is folded in */
RPT_HD rpt_gathered_info gather_info_begin() {
    rpt_gathered_info g;
    g.with_moments = 1u; g.nonuniform = 0u; g.samples_min = 0xffffffffu; g.samples_max = 0u; g.bad_trailers = 0u;
    g.reserved[0] = g.reserved[1] = g.reserved[2] = 0u;
    return g;
}
/* one rank's trailer into the info words: or / min / max / a count, so the result does not depend on the order.  A rank that owns no pixel has nothing
 * in the image: its counts say nothing about it (its format word is still checked). */
RPT_HD void gather_fold(rpt_gathered_info &g, uint4 t) {
    if (t.x != RPT_GATHER_FORMAT) { g.bad_trailers += 1u; return; }
    if (t.w == 0u) return;
    g.nonuniform |= t.y ? 1u : 0u;
    g.samples_min = t.z < g.samples_min ? t.z : g.samples_min;
    g.samples_max = t.z > g.samples_max ? t.z : g.samples_max;
}
/* after the last trailer: ranks whose uniform counts differ make the image's counts non-uniform; no rank with pixels: min = max = 0 */
RPT_HD void gather_info_end(rpt_gathered_info &g) {
    if (g.samples_min > g.samples_max) g.samples_min = g.samples_max = 0u;
    if (g.samples_min != g.samples_max) g.nonuniform = 1u;
}

/* the kernels: for the one unit that launches them (rpt_comm.hip defines RPT_GATHER_KERNELS); the host hooks of rpt_debug.hip take the functions above */
#ifdef RPT_GATHER_KERNELS
/* The snapshot of a gather, on the render stream: accumulator block and moments record into the two halves of the rank's slot — one float4 load and one
 * float4 store per lane and record, consecutive lanes on consecutive pixels — and the trailer, whose values are kernel arguments: captured when the gather
 * is enqueued, written stream-ordered behind the batch.  The grid covers max(n_pixels, 1): a rank without pixels still writes its trailer. */
static __global__ __launch_bounds__(RPT_BLOCK) void k_gather_pack(const float4 *accum, const float4 *moments, uint32_t n_pixels, GatherLayout l, uint4 trailer, float4 *send) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i == 0u) *reinterpret_cast<uint4 *>(send + l.trailer_at) = trailer;
    if (i >= n_pixels) return;
    send[i] = accum[i];
    send[l.moments_at + i] = moments[i];
}

/* The root's un-tile, on the gather's stream: blockIdx.y = the rank, blockIdx.x covers its stride.  A lane loads its map word once (0xffffffff: padding,
 * nobody's) and scatters both records of its element; lane 0 of the launch folds the `world` trailers in rank order into the info words. */
static __global__ __launch_bounds__(RPT_BLOCK) void k_gather_untile2(const uint32_t *map, const float4 *gathered, GatherLayout l, uint32_t world, uint32_t width, float4 *full_image,
                                                                     float4 *full_moments, rpt_gathered_info *info) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x, r = blockIdx.y;
    if (i == 0u && r == 0u) {
        rpt_gathered_info g = gather_info_begin();
        for (uint32_t k = 0; k < world; ++k) gather_fold(g, *reinterpret_cast<const uint4 *>(gathered + (size_t)k * l.slot + l.trailer_at));
        gather_info_end(g);
        *info = g;
    }
    if (i >= l.stride) return;
    const uint32_t pxy = map[(size_t)r * l.stride + i];
    if (pxy == 0xffffffffu) return;
    const float4 *slot = gathered + (size_t)r * l.slot;
    const size_t at = rpt_pixel_index(pxy, width);
    full_image[at] = slot[i];
    full_moments[at] = slot[l.moments_at + i];
}
#endif

#endif /* RPT_K_GATHER_H */
