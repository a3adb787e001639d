/*
 * k_firefly.h — the firefly clamp in front of rpt_denoise_variance and rpt_denoise_temporal (include/rpt/rpt.h rpt_denoise_var_params clamp_scale,
 * clamp_floor, clamp_radius): a pixel whose BRIGHTEST SAMPLE (the moments record's m.w, k_moments.h) exceeds what any other pixel of its window has seen
 * gets that one sample replaced by the limit, in its mean and in its record, before the mean is demodulated and before anything is blended or filtered.
 * Opt-in (clamp_scale == 0: the kernels of k_denoise.h / k_temporal.h are launched, untouched); the accumulator, the rng and the moments record are only
 * read.  As in k_denoise.h the per-pixel arithmetic is RPT_HD code that the device kernels and the host builds (rpt_debug_firefly_host,
 * rpt_debug_denoise_variance_host, rpt_debug_denoise_temporal_host) share — ff_tap, ff_offer and ff_apply; ff_pixel is the whole rule, as the host builds
 * call it — f32, no contraction, IEEE division — so they agree bit for bit, and
 * tests/firefly_ref.py restates it in numpy with the same operation order.  On the device the window is read out of LDS, where each workgroup stages the
 * (b, kind) of its pixels and their halo once (ff_stage, ff_window_lds: the same taps in the same order, so the same B); reading each tap where it lies, through
 * the caches, was built first and is 1.01 to 1.72 times slower (profiles/r16_firefly.txt).
 *
 * Pixel p: c_p = its mean in radiance units (sum.rgb / count_p), count_p = its own .w while the counts are non-uniform, else the uniform count, m_p its
 * record, kind_p its guide kind.  "Demodulated" is what the call decides (base.iterations != 0 && base.demodulate != 0).
 *   Ya_q  = mo_luminance(dn_albedo_floor(albedo_q)) where demodulated, else 1;   b(q) = m_q.w / Ya_q
 *   taps  q = p + (dx, dy), |dx|, |dy| <= clamp_radius, q != p, dy outer, dx inner, both ascending.  A tap is eligible if it is inside the image, of p's
 *         kind, has m_q.z >= 1 and a finite b(q): a NaN or an infinity never enters.
 *   B     = the largest b(q) over the eligible taps; no eligible tap: the pixel is untouched
 *   L     = max(clamp_scale * B, clamp_floor) * Ya_p
 *   p is CLAMPED iff  m_p.z >= 1,  m_p.z == count_p (a resumed accumulator — rpt_reset with accum_init — or a caller's record that counts differently is
 *         left alone),  m_p.x, m_p.y, m_p.w and L are finite,  m_p.x > 0  and  m_p.w > L.  Then, with w = m_p.w, n = m_p.z:
 *           x'  = (m.x - w) + L             a negative x' becomes 0
 *           y'  = (m.y - w * w) + L * L     a negative y' becomes 0
 *           rho = x' / m.x                  above 1 it becomes 1
 *           c'  = c * rho per channel,  m' = (x', y', n, L)
 * and everything downstream (demodulation, dn_prepare_variance, tp_pixel, the passes) runs unchanged on (c', m').
 *
 * LIMITS.  Only a pixel's ONE brightest sample is clamped: a pixel with two spikes keeps the second.  The chroma of the removed part is assumed to be the
 * pixel's mean chroma (the record holds luminance only).  Two adjacent spikes of like size shield each other: each is the other's B.  The clamp is
 * BIASED: it removes energy, and where almost every lit sample is rare it removes a lot (profiles/r16_firefly_quality.txt, the "lost" column).
 * y' cancels where the spike dominated m.y.  With u = 2^-24: w w rounds (u w^2), the difference rounds (u |m.y - w^2|), L carries e_L (b = w_q / Ya_q, scale * B
 * and * Ya_p: 9u where demodulated — Ya is three products and two sums, 3u, and enters twice — else u) and enters L L twice, which rounds ((2 e_L + u) L^2), and
 * the sum rounds (u y'):
 *     |y' - exact| <= D = u w^2 + u |m.y - w^2| + (2 e_L + u) L^2 + u y'      (and products of two roundings, below 32 u D)
 * Where the spike dominated and the limit is well below it — |m.y - w^2| <= w^2 / 4 and L <= w / 4 — D < 3 u w^2; with a limit near w (two spikes of like size,
 * a large clamp_scale) the L L term alone is up to 19 u w^2 where demodulated, 3 u w^2 where not.  The variance of the mean that dn_prepare_variance takes
 * from m' is off by up to D over n (n - 1) — beside mo_variance_of_mean's own bound (k_moments.h), and beside m.y itself having been summed in f32.
 * Unclamped, that pixel's variance was of the order w^2 / n^2.  tests/test_denoise_firefly.py holds the host build to D, and to 3 u w^2 under its premise,
 * against float64.
 */
#ifndef RPT_K_FIREFLY_H
#define RPT_K_FIREFLY_H

#include "k_temporal.h"

#define RPT_FF_MAX_RADIUS 3u

/* what a call needs of the clamp parameters and of the images the window reads.  `moments` is read at inverse[at] where inverse != null (the context's
 * tile-major record through the cached inverse map, as k_dn_temporal reads it), else at the row-major `at`; g1 = (position | kind) and albedo are row-major */
struct FfView {
    uint32_t width, height;
    uint32_t radius;               /* 1..3 */
    uint32_t demodulated;
    float scale, floor;
    const float4 *moments;
    const uint32_t *inverse;
    const float4 *g1;
    const float4 *albedo;
};

struct FfOut { F3 c; float4 m; bool clamped; };

/* Ya of a pixel: 1 where the call does not demodulate */
RPT_HD float ff_albedo_luminance(const FfView &fv, size_t at) {
    if (fv.demodulated == 0u) return 1.0f;
    const float4 al = fv.albedo[at];
    const F3 a = dn_albedo_floor(f3(al.x, al.y, al.z));
    return mo_luminance(a.x, a.y, a.z);
}

/* the window's running maximum: B over the eligible taps seen so far, in the order they are offered */
struct FfMax { bool any; float B; };
RPT_HD void ff_offer(FfMax &mx, float b) {
    if (!mx.any || b > mx.B) mx.B = b;
    mx.any = true;
}

/* what a tap offers: b(q), or +inf (never eligible: a finite b is what enters) where the record is unsampled or b is not finite */
RPT_HD float ff_tap(const FfView &fv, size_t aq) {
    const float4 mq = fv.moments[fv.inverse ? (size_t)fv.inverse[aq] : aq];
    if (!(mq.z >= 1.0f)) return rptm::u2f(0x7f800000u);
    const float b = mq.w / ff_albedo_luminance(fv, aq);
    return rptm::finiter(b) ? b : rptm::u2f(0x7f800000u);
}

/* the window of pixel (x, y), its taps read where they lie: dy outer, dx inner, both ascending */
RPT_HD FfMax ff_window(const FfView &fv, uint32_t x, uint32_t y) {
    FfMax mx{false, 0.0f};
    const uint32_t kind_p = rptm::f2u(fv.g1[(size_t)y * fv.width + x].w);
    const int r = (int)fv.radius;
    for (int dy = -r; dy <= r; ++dy) {
        const int qy = (int)y + dy;                                                 /* (extents <= 65535) */
        if (qy < 0 || qy >= (int)fv.height) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const int qx = (int)x + dx;
            if (qx < 0 || qx >= (int)fv.width || (dx == 0 && dy == 0)) continue;
            const size_t aq = (size_t)qy * fv.width + (size_t)qx;
            if (rptm::f2u(fv.g1[aq].w) != kind_p) continue;
            const float b = ff_tap(fv, aq);
            if (rptm::finiter(b)) ff_offer(mx, b);
        }
    }
    return mx;
}

/* One pixel, its window's maximum known: c = its mean in radiance units, count = the count that mean was divided by, m = its record.  The rule of the file's
 * head comment from L on. */
RPT_HD FfOut ff_apply(const FfView &fv, uint32_t x, uint32_t y, const FfMax &mx, F3 c, float count, const float4 &m) {
    FfOut o{c, m, false};
    if (!mx.any) return o;
    const float sB = fv.scale * mx.B;
    const float L = (sB > fv.floor ? sB : fv.floor) * ff_albedo_luminance(fv, (size_t)y * fv.width + x);
    const float w = m.w, n = m.z;
    if (!(n >= 1.0f) || n != count) return o;
    if (!rptm::finiter(m.x) || !rptm::finiter(m.y) || !rptm::finiter(w) || !rptm::finiter(L)) return o;
    if (!(m.x > 0.0f) || !(w > L)) return o;
    float x1 = (m.x - w) + L;
    if (x1 < 0.0f) x1 = 0.0f;
    float y1 = (m.y - w * w) + L * L;
    if (y1 < 0.0f) y1 = 0.0f;
    float rho = x1 / m.x;
    if (rho > 1.0f) rho = 1.0f;
    o.c = f3(c.x * rho, c.y * rho, c.z * rho);
    o.m = make_float4(x1, y1, n, L);
    o.clamped = true;
    return o;
}

/* One pixel: the rule of the file's head comment (the host builds; the device reads the window out of LDS, below, and calls ff_apply as this does) */
RPT_HD FfOut ff_pixel(const FfView &fv, uint32_t x, uint32_t y, F3 c, float count, const float4 &m) {
    return ff_apply(fv, x, y, ff_window(fv, x, y), c, count, m);
}

/* The window out of LDS.  A workgroup is 64 x 4 pixels (a wave a 64 x 1 row segment), so with the halo its windows cover at most 70 x 10 pixels, and each of
 * them is a tap of up to 48 windows: the workgroup stages every covered pixel's (b, kind) ONCE — 700 entries of 8 bytes, rows 70 entries apart whatever the
 * radius, 2.7 entries per pixel at radius 3 and 1.5 at radius 1 against 48 and 8 tap reads — and each lane then reads its taps with one 8-byte LDS read
 * each, neighbouring lanes neighbouring entries (no bank conflict).  A pixel outside the image is staged as +inf, as ff_tap stages an ineligible one, so the
 * window loop needs no bounds; same taps, same order, same b as ff_window, hence the same B bit for bit. */
#define RPT_FF_TILE_W 70u
#define RPT_FF_TILE_H 10u
__device__ __forceinline__ void ff_stage(const FfView &fv, float2 *tile) {
    const int r = (int)fv.radius;
    const int x0 = (int)(blockIdx.x * 64u) - r, y0 = (int)(blockIdx.y * 4u) - r;
    const uint32_t tw = 64u + 2u * fv.radius, th = 4u + 2u * fv.radius;
    for (uint32_t i = threadIdx.x; i < RPT_FF_TILE_W * RPT_FF_TILE_H; i += 256u) {
        const uint32_t ty = i / RPT_FF_TILE_W, tx = i - ty * RPT_FF_TILE_W;
        if (tx >= tw || ty >= th) continue;
        const int qx = x0 + (int)tx, qy = y0 + (int)ty;
        float2 e = make_float2(rptm::u2f(0x7f800000u), 0.0f);
        if (qx >= 0 && qx < (int)fv.width && qy >= 0 && qy < (int)fv.height) {
            const size_t aq = (size_t)qy * fv.width + (size_t)qx;
            e = make_float2(ff_tap(fv, aq), fv.g1[aq].w);
        }
        tile[i] = e;
    }
}
__device__ __forceinline__ FfMax ff_window_lds(const FfView &fv, const float2 *tile, uint32_t kind_p) {
    FfMax mx{false, 0.0f};
    const uint32_t r = fv.radius, lx = threadIdx.x & 63u, ly = threadIdx.x >> 6;
    for (uint32_t ty = ly; ty <= ly + 2u * r; ++ty)
        for (uint32_t tx = lx; tx <= lx + 2u * r; ++tx) {
            if (tx == lx + r && ty == ly + r) continue;
            const float2 e = tile[ty * RPT_FF_TILE_W + tx];
            if (rptm::f2u(e.y) == kind_p && rptm::finiter(e.x)) ff_offer(mx, e.x);
        }
    return mx;
}

/* *counter += the lanes of the wave whose flag is set: one ballot and one integer atomic per wave (the order does not matter) */
__device__ __forceinline__ void ff_count_wave(bool flag, unsigned long long *counter) {
    const unsigned long long mask = rpt_ballot(flag);
    if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(counter, (unsigned long long)__popcll(mask));
}

/* one pixel of a clamp kernel: its sums, its mean (OWN: by its own .w), its window out of the staged tile, ff_apply */
template <bool OWN>
__device__ __forceinline__ FfOut ff_pixel_lds(const FfView &fv, const float2 *tile, uint32_t x, uint32_t y, const float4 *sums, const uint32_t *inverse, float sample_count) {
    const size_t at = (size_t)y * fv.width + x;
    const float4 a = sums[inverse ? (size_t)inverse[at] : at];
    const F3 mean = OWN ? mean_own(a) : f3(a.x / sample_count, a.y / sample_count, a.z / sample_count);
    const FfMax mx = ff_window_lds(fv, tile, rptm::f2u(fv.g1[at].w));
    return ff_apply(fv, x, y, mx, mean, OWN ? a.w : sample_count, fv.moments[fv.inverse ? (size_t)fv.inverse[at] : at]);
}

/* k_dn_prepare_var with the clamp in front: the mean (OWN: every pixel by its own .w), the clamp, then the demodulation and the variance of k_dn_prepare_var on
 * (c', m').  The mapping of k_dn_pass — a wave is a 64 x 1 row segment, a workgroup 64 x 4 pixels; `inverse` != null: `sums` is tile-major and inverse[at] is
 * the element of row-major pixel `at` (the record: FfView).  5600 bytes of LDS, no scratch. */
template <bool OWN>
__global__ __launch_bounds__(256) void k_dn_prepare_var_clamp(FfView fv, const float4 *sums, const uint32_t *inverse, float sample_count, float4 *out, unsigned long long *clamped) {
    __shared__ float2 tile[RPT_FF_TILE_W * RPT_FF_TILE_H];
    ff_stage(fv, tile);
    __syncthreads();
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    bool hit = false;
    if (x < fv.width && y < fv.height) {
        const size_t at = (size_t)y * fv.width + x;
        const FfOut f = ff_pixel_lds<OWN>(fv, tile, x, y, sums, inverse, sample_count);
        F3 c = f.c, al = f3s(1.0f);
        if (fv.demodulated != 0u) { al = xyz4(fv.albedo[at]); c = dn_demodulate(c, al); }
        const float v = dn_prepare_variance(f.m, fv.demodulated != 0u, al);
        out[at] = make_float4(c.x, c.y, c.z, v);
        hit = f.clamped;
    }
    ff_count_wave(hit, clamped);
}

/* k_dn_temporal with the clamp in front: tp_pixel takes the demodulated c' as e_cur and m' as m, so a spike is clamped before it can enter the history */
template <bool OWN>
__global__ __launch_bounds__(256) void k_dn_temporal_clamp(FfView fv, TpView vw, TpPrev pv, const float4 *sums, const uint32_t *inverse, float sample_count, const float4 *g0, float4 *out,
                                                           float4 *h_out, float2 *mu_out, float *t_out, unsigned long long *with_history, unsigned long long *clamped) {
    __shared__ float2 tile[RPT_FF_TILE_W * RPT_FF_TILE_H];
    ff_stage(fv, tile);
    __syncthreads();
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    bool reused = false, hit = false;
    if (x < fv.width && y < fv.height) {
        const size_t at = (size_t)y * fv.width + x;
        const FfOut f = ff_pixel_lds<OWN>(fv, tile, x, y, sums, inverse, sample_count);
        F3 c = f.c, al = f3s(1.0f);
        if (fv.demodulated != 0u) { al = xyz4(fv.albedo[at]); c = dn_demodulate(c, al); }
        const TpOut o = tp_pixel(vw, pv, x, y, c, f.m, g0[at], fv.g1[at], fv.demodulated != 0u, al);
        out[at] = make_float4(o.e.x, o.e.y, o.e.z, o.v);
        h_out[at] = make_float4(o.e.x, o.e.y, o.e.z, o.N);
        mu_out[at] = make_float2(o.mu1, o.mu2);
        t_out[at] = o.T;
        reused = o.reused;
        hit = f.clamped;
    }
    ff_count_wave(reused, with_history);
    ff_count_wave(hit, clamped);
}

#endif /* RPT_K_FIREFLY_H */
