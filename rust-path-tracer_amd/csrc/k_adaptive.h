/*
 * k_adaptive.h — rendering CHOSEN pixels (include/rpt/rpt.h rpt_render_pixels, rpt_render_adaptive): the selection rule, the ordered compaction of the
 * selected pixels and the copies into and out of the compact per-pixel state a masked pass renders on (rpt_adaptive.hip), and the per-pixel division
 * by a pixel's OWN sample count that the read-outs use once counts differ (rpt_resolve, rpt_denoise).  No kernel of the wavefront pipeline is touched:
 * a pass gathers (pixel_xy, rng, accum, moments) of the selected pixels into arrays of their own, the unchanged pipeline runs on them as it runs on a
 * rank that owns few pixels, and the records go back where they came from.
 *
 * Compaction in ASCENDING pixel order — count per workgroup (ballot + popcount), exclusive scan of the workgroup counts, scatter — so the survivors keep
 * the tile-major order (their 8 x 8 blocks stay together in a wave) and the result does not depend on the order waves arrive in; no atomic-append list.
 * The per-pixel functions are RPT_HD: the host build (rpt_debug_adaptive_select_host) is the same text in a loop.
 * rpt_render_adaptive_window selects by a pixel's NEIGHBOURHOOD instead (k_ad_window below, one workgroup per owned tile; its per-pixel and per-row pieces
 * are RPT_HD too: rpt_debug_adaptive_window_host) and feeds the same compaction through the flag bytes.
 */
#ifndef RPT_K_ADAPTIVE_H
#define RPT_K_ADAPTIVE_H

#include "../../include/rpt/rpt.h"       /* RPT_TILE */
#include "k_common.h"
#include "k_moments.h"
#include "k_tonemap.h"

/* The selection rule of rpt_render_adaptive: a pixel gets `batch` more samples while its noise is not at or below the threshold (noise_above: an unmeasured
 * record, +inf, and a NaN are selected) and the batch still fits under the cap.  m.z is the pixel's own count in the moments record; batch and cap are the
 * target's batch_samples and max_samples as f32. */
RPT_HD bool adaptive_selected(const float4 &m, float threshold, float batch, float cap) { return noise_above(noise_rel(m), threshold) && m.z + batch <= cap; }

/* a pixel's sum divided by its OWN count (accum.w); a pixel without a sample resolves to 0 */
RPT_HD F3 mean_own(const float4 &a) { return a.w == 0.0f ? f3(0.0f, 0.0f, 0.0f) : f3(a.x / a.w, a.y / a.w, a.z / a.w); }

/* what a selection reports to the host: n_active is the pass's one read (4 bytes); a noise selection adds the counts of rpt_noise_count and the range of m.z */
struct AdResult {
    uint32_t n_active;
    uint32_t z_min_inv, z_max;             /* ~min and max of (uint32_t)m.z over the owned pixels (both taken with atomicMax: the record starts as zeros) */
    uint32_t pad;
    unsigned long long pixels, measured, above;
};

/* the per-pixel arrays of a context, or the compact ones of a pass (moments: null when they are off) */
struct AdPixels {
    uint32_t *pixel_xy;
    uint2 *rng;
    float4 *accum;
    float4 *moments;
};

/* source (a): the caller's row-major byte mask, read through pixel_xy as k_reset_gather reads the seeds.  Every lane of the workgroup calls select(). */
struct AdMaskSel {
    const uint32_t *pixel_xy;
    const uint8_t *mask;
    uint32_t width;
    __device__ __forceinline__ bool select(uint32_t s, bool in_range, AdResult *) const { return in_range && mask[rpt_pixel_index(pixel_xy[s], width)] != 0u; }
};
/* source (b): the rule above on the moments record; also counts what rpt_noise_count counts (one ballot and one integer atomic per wave and non-zero count)
 * and reduces the range of m.z (butterfly over the wave, one atomic pair per wave) */
struct AdNoiseSel {
    const float4 *moments;
    float threshold, batch, cap;
    __device__ __forceinline__ bool select(uint32_t s, bool in_range, AdResult *res) const {
        bool measured = false, above = false, chosen = false;
        uint32_t lo = 0xffffffffu, hi = 0u;
        if (in_range) {
            const float4 m = moments[s];
            measured = mo_measured(m);
            above = measured && noise_above(noise_rel(m), threshold);
            chosen = adaptive_selected(m, threshold, batch, cap);
            lo = hi = m.z >= 0.0f ? (uint32_t)m.z : 0u;
        }
        const unsigned long long mi = rpt_ballot(in_range), mm = rpt_ballot(measured), ma = rpt_ballot(above);
#pragma unroll
        for (int d = 1; d < RPT_WAVE; d <<= 1) {
            const uint32_t olo = (uint32_t)__shfl_xor((int)lo, d, RPT_WAVE), ohi = (uint32_t)__shfl_xor((int)hi, d, RPT_WAVE);
            lo = olo < lo ? olo : lo;
            hi = ohi > hi ? ohi : hi;
        }
        if ((threadIdx.x & (RPT_WAVE - 1u)) == 0u && mi != 0ull) {
            atomicAdd(&res->pixels, (unsigned long long)__popcll(mi));
            if (mm != 0ull) atomicAdd(&res->measured, (unsigned long long)__popcll(mm));
            if (ma != 0ull) atomicAdd(&res->above, (unsigned long long)__popcll(ma));
            atomicMax(&res->z_min_inv, ~lo);
            atomicMax(&res->z_max, hi);
        }
        return chosen;
    }
};

/* step 1 + 2a: the flag of every owned pixel (a byte, kept for the scatter) and the number of flagged pixels of each workgroup */
template <typename Sel>
static __global__ __launch_bounds__(RPT_BLOCK) void k_ad_count(Sel sel, uint32_t n_pixels, uint8_t *flags, uint32_t *wg_count, AdResult *res) {
    __shared__ uint32_t wave_n[RPT_BLOCK / RPT_WAVE];
    const uint32_t s = blockIdx.x * RPT_BLOCK + threadIdx.x;
    const bool in_range = s < n_pixels;
    const bool flag = sel.select(s, in_range, res);
    if (in_range) flags[s] = flag ? 1u : 0u;
    const unsigned long long m = rpt_ballot(flag);
    if ((threadIdx.x & (RPT_WAVE - 1u)) == 0u) wave_n[threadIdx.x / RPT_WAVE] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (uint32_t w = 0; w < RPT_BLOCK / RPT_WAVE; ++w) total += wave_n[w];
        wg_count[blockIdx.x] = total;
    }
}

/* ---- the window rule of rpt_render_adaptive_window: a pixel is selected while ANY pixel of its window is still noisy ---------------------------------------
 *   above(q)    = noise_above(noise_rel(m_q), threshold)                 (an unmeasured record, +inf and a NaN are above)
 *   fits(p)     = m_p.z + batch <= cap
 *   selected(p) = fits(p) && some q with |x_q - x_p| <= radius, |y_q - y_p| <= radius, inside the image and inside p's OWN RPT_TILE x RPT_TILE tile, is above
 * radius 0 is adaptive_selected.  The window is clipped to the tile: a rank holds the records of its own tiles only, so the selection does not depend on the
 * partition.  A tile's `above` mask is RPT_TILE row words of 64 bits (bit x of word y: the pixel at (x, y) from the tile's origin; rows and bits outside the
 * tile or the image stay 0) and the dilation is integer work on those words: ad_dilate_row across, ad_dilate_rows down.  fits is applied AFTER the dilation:
 * a pixel at the cap is never selected, yet spreads. */
static_assert(RPT_TILE == 64 && RPT_WAVE == 64, "a tile row is one 64-bit word, and a wave's ballot is one 8 x 8 block of a full tile");

RPT_HD bool ad_above(const float4 &m, float threshold) { return noise_above(noise_rel(m), threshold); }
RPT_HD bool ad_fits(const float4 &m, float batch, float cap) { return m.z + batch <= cap; }
/* OR of the row shifted by -radius .. radius (bits shifted past either end of the word are lost: no wrap) */
RPT_HD unsigned long long ad_dilate_row(unsigned long long row, uint32_t radius) {
    unsigned long long h = row;
    for (uint32_t d = 1u; d <= radius; ++d) h |= (row << d) | (row >> d);
    return h;
}
/* OR of the RPT_TILE words h[] over rows y - radius .. y + radius, clipped to the tile */
RPT_HD unsigned long long ad_dilate_rows(const unsigned long long *h, uint32_t y, uint32_t radius) {
    const uint32_t lo = y > radius ? y - radius : 0u, hi = y + radius < RPT_TILE - 1u ? y + radius : RPT_TILE - 1u;
    unsigned long long v = 0ull;
    for (uint32_t q = lo; q <= hi; ++q) v |= h[q];
    return v;
}

/* an owned tile in the rank's pixel order (rpt_hip.hip rpt_build_tile_table, beside rpt_build_pixel_order): its pixels are the entries first .. first + count - 1 */
struct AdTile {
    uint32_t first, count;
    uint32_t origin;                       /* x | y << 16 of its top left pixel */
    uint32_t pad;
};

/* The selection of the window rule: ONE WORKGROUP PER OWNED TILE.  (1) every pixel's `above` bit into the tile's row words in LDS — on a full tile a wave is
 * one 8 x 8 block and its ballot is eight row bytes, stored as bytes without atomics; a partial tile (right and bottom edge: narrower blocks) goes through
 * pixel_xy and an LDS atomic OR — together with the counts and the range of m.z that AdNoiseSel::select reduces, which come out the same; (2) 64 lanes
 * dilate the 64 rows across, then down; (3) every pixel reads its own bit, ANDs fits and writes flags[s].  No scratch, no global atomics but the counts',
 * 2 x 64 x 8 = 1024 bytes of LDS. */
static __global__ __launch_bounds__(RPT_BLOCK) void k_ad_window(const AdTile *tiles, const uint32_t *pixel_xy, const float4 *moments, uint32_t n_pixels, float threshold, float batch, float cap,
                                                                uint32_t radius, uint8_t *flags, AdResult *res) {
    __shared__ unsigned long long rows[RPT_TILE], wide[RPT_TILE];
    const AdTile t = tiles[blockIdx.x];
    const uint32_t tx = t.origin & 0xffffu, ty = t.origin >> 16, lane = threadIdx.x & (RPT_WAVE - 1u);
    const bool full = t.count == RPT_TILE * RPT_TILE;
    if (threadIdx.x < RPT_TILE) rows[threadIdx.x] = 0ull;
    __syncthreads();
    uint32_t n_in = 0u, n_measured = 0u, n_above = 0u, lo = 0xffffffffu, hi = 0u;
    for (uint32_t base = 0u; base < t.count; base += RPT_BLOCK) {
        const uint32_t i = base + threadIdx.x, s = t.first + i;
        const bool in_range = i < t.count && s < n_pixels;
        bool measured = false, above = false;
        if (in_range) {
            const float4 m = moments[s];
            measured = mo_measured(m);
            above = ad_above(m, threshold);
            const uint32_t z = m.z >= 0.0f ? (uint32_t)m.z : 0u;
            lo = z < lo ? z : lo;
            hi = z > hi ? z : hi;
        }
        const unsigned long long ma = rpt_ballot(above);
        n_in += (uint32_t)__popcll(rpt_ballot(in_range));
        n_measured += (uint32_t)__popcll(rpt_ballot(measured));
        n_above += (uint32_t)__popcll(rpt_ballot(measured && above));
        if (full) {
            const uint32_t block = i / RPT_WAVE, bx = block & 7u, by = block >> 3;                   /* (the wave's 8 x 8 block: rpt_build_pixel_order) */
            if (lane < 8u) reinterpret_cast<uint8_t *>(rows)[(by * 8u + lane) * 8u + bx] = (uint8_t)(ma >> (8u * lane));
        } else if (above) {
            const uint32_t pxy = pixel_xy[s], x = (pxy & 0xffffu) - tx, y = (pxy >> 16) - ty;
            if (x < RPT_TILE && y < RPT_TILE) atomicOr(&rows[y], 1ull << x);
        }
    }
#pragma unroll
    for (int d = 1; d < RPT_WAVE; d <<= 1) {
        const uint32_t olo = (uint32_t)__shfl_xor((int)lo, d, RPT_WAVE), ohi = (uint32_t)__shfl_xor((int)hi, d, RPT_WAVE);
        lo = olo < lo ? olo : lo;
        hi = ohi > hi ? ohi : hi;
    }
    if (lane == 0u && n_in != 0u) {
        atomicAdd(&res->pixels, (unsigned long long)n_in);
        if (n_measured != 0u) atomicAdd(&res->measured, (unsigned long long)n_measured);
        if (n_above != 0u) atomicAdd(&res->above, (unsigned long long)n_above);
        atomicMax(&res->z_min_inv, ~lo);
        atomicMax(&res->z_max, hi);
    }
    __syncthreads();
    if (threadIdx.x < RPT_TILE) wide[threadIdx.x] = ad_dilate_row(rows[threadIdx.x], radius);
    __syncthreads();
    if (threadIdx.x < RPT_TILE) rows[threadIdx.x] = ad_dilate_rows(wide, threadIdx.x, radius);
    __syncthreads();
    for (uint32_t base = 0u; base < t.count; base += RPT_BLOCK) {
        const uint32_t i = base + threadIdx.x, s = t.first + i;
        if (i >= t.count || s >= n_pixels) continue;
        const uint32_t pxy = pixel_xy[s], x = (pxy & 0xffffu) - tx, y = (pxy >> 16) - ty;
        const bool near = x < RPT_TILE && y < RPT_TILE && ((rows[y] >> x) & 1ull) != 0ull;
        flags[s] = near && ad_fits(moments[s], batch, cap) ? 1u : 0u;
    }
}

/* source (c): the flag bytes k_ad_window wrote, into the unchanged ordered compaction */
struct AdFlagSel {
    const uint8_t *flags;
    __device__ __forceinline__ bool select(uint32_t s, bool in_range, AdResult *) const { return in_range && flags[s] != 0u; }
};

/* step 2b: exclusive scan of the workgroup counts by ONE workgroup (a contiguous run of counts per thread, the 256 run sums scanned by thread 0), and their
 * total: n_active.  The counts are few — a workgroup per 256 pixels — and the scan is off the hot path. */
static __global__ __launch_bounds__(RPT_BLOCK) void k_ad_scan(const uint32_t *wg_count, uint32_t n_blocks, uint32_t *wg_offset, AdResult *res) {
    __shared__ uint32_t part[RPT_BLOCK];
    const uint32_t per = (n_blocks + RPT_BLOCK - 1u) / RPT_BLOCK;
    const uint32_t lo = threadIdx.x * per < n_blocks ? threadIdx.x * per : n_blocks, hi = lo + per < n_blocks ? lo + per : n_blocks;
    uint32_t sum = 0u;
    for (uint32_t i = lo; i < hi; ++i) sum += wg_count[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t running = 0u;
        for (uint32_t t = 0; t < RPT_BLOCK; ++t) {
            const uint32_t v = part[t];
            part[t] = running;
            running += v;
        }
        res->n_active = running;
    }
    __syncthreads();
    uint32_t at = part[threadIdx.x];
    for (uint32_t i = lo; i < hi; ++i) {
        wg_offset[i] = at;
        at += wg_count[i];
    }
}

/* step 2c: flagged pixel s becomes entry i of the compact arrays, i = the flagged pixels below s: active[i] = s and the copies of its records.
 * capacity: what the compact arrays hold (>= n_active, checked all the same) */
static __global__ __launch_bounds__(RPT_BLOCK) void k_ad_scatter(AdPixels whole, uint32_t n_pixels, const uint8_t *flags, const uint32_t *wg_offset, uint32_t capacity, uint32_t *active,
                                                                 AdPixels compact) {
    __shared__ uint32_t wave_n[RPT_BLOCK / RPT_WAVE];
    const uint32_t s = blockIdx.x * RPT_BLOCK + threadIdx.x, wave = threadIdx.x / RPT_WAVE;
    const bool flag = s < n_pixels && flags[s] != 0u;
    const unsigned long long m = rpt_ballot(flag);
    if ((threadIdx.x & (RPT_WAVE - 1u)) == 0u) wave_n[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t i = wg_offset[blockIdx.x] + rpt_lane_rank(m);
    for (uint32_t w = 0; w < wave; ++w) i += wave_n[w];
    if (!flag || i >= capacity) return;
    active[i] = s;
    compact.pixel_xy[i] = whole.pixel_xy[s];
    compact.rng[i] = whole.rng[s];
    compact.accum[i] = whole.accum[s];
    if (whole.moments) compact.moments[i] = whole.moments[s];
}

/* step 4: the compact records back to the pixels they belong to, stream-ordered behind the batch */
static __global__ __launch_bounds__(RPT_BLOCK) void k_ad_scatter_back(AdPixels compact, const uint32_t *active, uint32_t n_active, uint32_t n_pixels, AdPixels whole) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n_active) return;
    const uint32_t s = active[i];
    if (s >= n_pixels) return;
    whole.rng[s] = compact.rng[i];
    whole.accum[s] = compact.accum[i];
    if (whole.moments) whole.moments[s] = compact.moments[i];
}

/* rpt_resolve while the counts are non-uniform: PixelResolve (k_image_order.h) with mean_own in place of sum / sample_count */
struct PixelResolveOwn {
    static constexpr size_t per_pixel = 3;
    const float4 *accum;
    uint32_t op;
    float *image;
    __device__ void operator()(uint32_t i, size_t at) const {
        const F3 c = tonemap(op, mean_own(accum[i]));
        float *rgb = image + 3u * at;
        rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
    }
};

#endif /* RPT_K_ADAPTIVE_H */
