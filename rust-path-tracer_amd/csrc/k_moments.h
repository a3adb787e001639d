/*
 * k_moments.h — per-pixel sample moments and the noise estimate derived from them (include/rpt/rpt.h rpt_set_moments, rpt_read_noise, rpt_noise_count,
 * rpt_render_to_noise).  Opt-in: a context with moments on keeps one float4 per owned pixel beside its accumulator, in the same tile-major pixel order,
 * updated by the completion kernel (k_complete.h k_complete_moments) once per finished sample, in sample order, with the radiance the accumulator gets.
 * The per-pixel arithmetic is the RPT_HD functions below — f32, no contraction, IEEE division and square root — which the device kernels and the host
 * build (rpt_debug_noise_host) both call, so the two agree bit for bit and tests/test_moments.py restates them in numpy with the same operation order.
 *
 *   m.x  sum of the samples' luminance Y        m.z  samples since the record was last zeroed
 *   m.y  sum of Y * Y                           m.w  the brightest sample
 * The f32 sum order is part of the result, as for the accumulator.
 */
#ifndef RPT_K_MOMENTS_H
#define RPT_K_MOMENTS_H

#include "rpt_math.h"

#define RPT_NOISE_MEAN_FLOOR 0.01f     /* added to |mean| in noise_rel: keeps black pixels finite */

/* Rec. 709 luminance of a radiance sample */
RPT_HD float mo_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

/* one finished sample of radiance (r, g, b) into the record (the product Y * Y is rounded, then added; a NaN never becomes the maximum) */
RPT_HD void mo_add(float4 &m, float r, float g, float b) {
    const float Y = mo_luminance(r, g, b);
    const float YY = Y * Y;
    m.x = m.x + Y;
    m.y = m.y + YY;
    m.z = m.z + 1.0f;
    m.w = Y > m.w ? Y : m.w;
}

/* a record is measured once it holds two samples (a variance exists) */
RPT_HD bool mo_measured(const float4 &m) { return m.z >= 2.0f; }

/* The standard error of the pixel's mean luminance relative to that mean: sqrt(max(0, sum(Y^2) - sum(Y)^2 / n) / (n (n - 1))) / (|mean| + 0.01).
 * +inf for a record that is not measured or whose sums are not finite.  An empirical variance: a pixel whose samples so far were all equal gives 0. */
RPT_HD float noise_rel(const float4 &m) {
    const float n = m.z;
    if (!mo_measured(m) || !rptm::finiter(m.x) || !rptm::finiter(m.y)) return rptm::u2f(0x7f800000u);
    const float mean = m.x / n;
    const float ss = m.y - (m.x * m.x) / n;
    const float v = ss / (n * (n - 1.0f));
    const float sem = rptm::sqrtr(v > 0.0f ? v : 0.0f);
    return sem / (__builtin_fabsf(mean) + RPT_NOISE_MEAN_FLOOR);
}

/* The empirical variance of the pixel's MEAN luminance (the square of noise_rel's standard error, in radiance units): max(0, sum(Y^2) - sum(Y)^2 / n) /
 * (n (n - 1)), the operations of noise_rel's `ss` and `v` lines in their order.  +inf — "unknown" — for a record that is not measured or whose sums are
 * not finite; a known variance is finite and >= 0 (mo_variance_known).  What rpt_denoise_variance filters by (k_denoise.h).
 * The one-pass difference cancels where a pixel's few samples nearly agree, so RELATIVELY the result can be off by anything there; absolutely it stays within
 * 2 * 2^-24 * sum(Y^2) / (n (n - 1)) + 2 * 2^-24 * v of the exact value for the record (tests/denoise_f64_cases.py derives it; 1.4 is the largest measured). */
RPT_HD float mo_variance_of_mean(const float4 &m) {
    const float n = m.z;
    if (!mo_measured(m) || !rptm::finiter(m.x) || !rptm::finiter(m.y)) return rptm::u2f(0x7f800000u);
    const float ss = m.y - (m.x * m.x) / n;
    return (ss > 0.0f ? ss : 0.0f) / (n * (n - 1.0f));
}
RPT_HD bool mo_variance_known(float v) { return rptm::finiter(v); }

/* what rpt_noise_count counts of a measured record: NOT (rel <= threshold), so a NaN counts as above */
RPT_HD bool noise_above(float rel, float threshold) { return !(rel <= threshold); }

#endif /* RPT_K_MOMENTS_H */
