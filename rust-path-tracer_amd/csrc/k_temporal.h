/*
 * k_temporal.h — temporal reuse in front of the variance-guided filter (include/rpt/rpt.h rpt_denoise_temporal): the history of the PREVIOUS view is
 * reprojected into the current one through the first-hit guides and blended with the current accumulator before the passes of k_denoise.h run.  Opt-in;
 * k_denoise.h, its kernels and its passes are not touched.  As there, the per-pixel arithmetic is ONE RPT_HD function (tp_pixel) that the device kernel
 * (k_dn_temporal) and the host build (rpt_debug_denoise_temporal_host) both call — f32, no contraction, IEEE division — so the two agree bit for bit, and
 * tests/temporal_ref.py restates it in numpy with the same operation order.
 *
 * History, per pixel, row-major:  h = (e_h.rgb | N)   e_h in the filter's units (demodulated where the passes demodulate), N an f32 sample count, 0 = none
 *                                 mu = (mu1, mu2)     per-sample first and second luminance moments, in radiance units
 * beside the g0 / g1 guide records of the view it was made under and that view's camera (position, rotation matrix).
 * THE HISTORY IS THE BLENDED IMAGE BEFORE THE PASSES, NOT THE FILTERED ONE: what is fed back is an average of samples, never a blur of a blur.
 *
 * Reprojection of a centre p with current guides (n_p, t_p, x_p, kind_p) into the previous view:
 *   d  = euler_prev^T (x_p - o),  o = ro_prev for hits, ro_cur for misses (the sky is at infinity: only the rotation moves it);  !(d.z > 0): no history
 *   ux = d.x / d.z,  uy = (d.y / d.z) / (H / W),  sx = ((ux + 1) / 2) W,  sy = (1 - (uy + 1) / 2) H       the inverse of camera_ray_centre (k_denoise.h)
 *   fx = sx - 0.5,  x0 = floor(fx),  a = fx - x0; fy, y0, b likewise;  !(-1 < fx < W && -1 < fy < H) (a NaN included): no history
 *   taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) in this order with w = (1-a)(1-b), a(1-b), (1-a)b, ab.  A tap q joins iff it is inside the
 *   image, its N > 0, its previous kind equals kind_p and — for non-misses — n_p . n_q >= normal_min and |n_p . (x_q - x_p)| / ((2 / W) t_p) <= plane_max
 *   (x_q, n_q: the PREVIOUS view's guides at q; a NaN fails either test).
 *   Wt = sum(w) over the joined taps;  !(Wt > 0.01): no history.  Else e_r, mu1_r, mu2_r = sum(w .) / Wt,  N_r = min(sum(w N) / Wt, max_history).
 *   Cameras equal bit for bit: the one tap is p itself with w = 1, still validated.
 * Blend with the current mean e_cur (rpt_denoise's) and moments record m, n_cur = m.z, T = N_r + n_cur:
 *   N_r > 0 fails (or e_cur is not finite)   e = e_cur, v = dn_prepare_variance(m), mu = (m.x / n_cur, m.y / n_cur), T = n_cur: rpt_denoise_variance bit for bit
 *   else                                     e = (N_r e_r + n_cur e_cur) / T,  mu1 = (N_r mu1_r + m.x) / T, mu2 likewise (a record whose m.x or m.y is not finite adds 0),
 *                                            v = max(0, mu2 - mu1 mu1) / (T - 1), known iff T >= 2 and mu1, mu2 are finite, else +inf; divided by Ya^2 where demodulated
 * The new history record is (e | T), (mu1, mu2); N = 0 instead of T where e is not finite.
 * No rule guards the COUNT: a record whose m.z is NaN or infinite (no render writes one; a caller's moments image can hold one) gives T = N_r + m.z and with
 * it a blended colour that is NaN although e_cur is finite (tests/test_denoise_f64.py shows it).  It leaves N = 0 behind like any colour that is not finite,
 * so it reaches no later blend; without history such a record gives e = e_cur as ever.
 */
#ifndef RPT_K_TEMPORAL_H
#define RPT_K_TEMPORAL_H

#include "k_denoise.h"
#include "k_adaptive.h"          /* mean_own: every pixel by its own count while the counts are non-uniform */

/* what a call needs of the two cameras and of rpt_temporal_params, worked out once on the host (the same f32 operations for the device and the host build) */
struct TpView {
    uint32_t width, height;
    uint32_t has_history;          /* a previous view exists (else every pixel takes the first branch of the blend) */
    uint32_t identity;             /* the previous camera's position and matrix equal the current ones bit for bit */
    float fw, fh, aspect;          /* (float)W, (float)H, (float)H / (float)W */
    float footprint;               /* 2 / W: times t_p it is the plane distance of one pixel footprint (k_denoise.h DnPass::plane_scale at sigma_plane * step = 1) */
    float max_history, normal_min, plane_max;
    float ro_cur[3], ro_prev[3];
    float euler_prev[9];           /* column-major, as DevConfig::euler */
};
RPT_HD TpView tp_view(uint32_t width, uint32_t height, float max_history, float normal_min, float plane_max) {
    TpView v{};
    v.width = width; v.height = height;
    v.fw = (float)width; v.fh = (float)height;
    v.aspect = (float)height / (float)width;
    v.footprint = 2.0f / (float)width;
    v.max_history = max_history; v.normal_min = normal_min; v.plane_max = plane_max;
    return v;
}

/* the previous view as a call reads it: all null / unused while has_history == 0 */
struct TpPrev {
    const float4 *h;               /* (e_h | N) */
    const float2 *mu;
    const float4 *g0, *g1;
};

struct TpSum { F3 e; float n, mu1, mu2, wt; };

/* one bilinear tap (qx, qy) of weight w into the sums, if it joins */
RPT_HD void tp_tap(const TpView &vw, const TpPrev &pv, int qx, int qy, float w, F3 n_p, F3 x_p, float plane, uint32_t kind_p, TpSum &s) {
    if (qx < 0 || qy < 0 || qx >= (int)vw.width || qy >= (int)vw.height) return;
    const size_t aq = (size_t)qy * vw.width + (size_t)qx;
    const float4 h = pv.h[aq];
    if (!(h.w > 0.0f)) return;
    const float4 b1 = pv.g1[aq];
    if (rptm::f2u(b1.w) != kind_p) return;
    if (kind_p != RPT_DN_KIND_MISS) {
        const float4 b0 = pv.g0[aq];
        if (!(dot3(n_p, f3(b0.x, b0.y, b0.z)) >= vw.normal_min)) return;
        if (!(rptm::absr(dot3(n_p, f3(b1.x, b1.y, b1.z) - x_p)) / plane <= vw.plane_max)) return;
    }
    const float2 m = pv.mu[aq];
    s.e = s.e + w * f3(h.x, h.y, h.z);
    s.n = s.n + w * h.w;
    s.mu1 = s.mu1 + w * m.x;
    s.mu2 = s.mu2 + w * m.y;
    s.wt = s.wt + w;
}

/* the screen position of x_p in the previous view, minus half a pixel: false = behind that camera or outside (-1, W) x (-1, H) */
RPT_HD bool tp_project(const TpView &vw, F3 x_p, uint32_t kind_p, float &fx, float &fy) {
    const F3 o = kind_p == RPT_DN_KIND_MISS ? f3(vw.ro_cur[0], vw.ro_cur[1], vw.ro_cur[2]) : f3(vw.ro_prev[0], vw.ro_prev[1], vw.ro_prev[2]);
    const F3 r = x_p - o;
    const float *m = vw.euler_prev;
    const F3 d = f3(dot3(f3(m[0], m[1], m[2]), r), dot3(f3(m[3], m[4], m[5]), r), dot3(f3(m[6], m[7], m[8]), r));
    if (!(d.z > 0.0f)) return false;
    const float ux = d.x / d.z, uy = (d.y / d.z) / vw.aspect;
    const float sx = ((ux + 1.0f) / 2.0f) * vw.fw, sy = (1.0f - (uy + 1.0f) / 2.0f) * vw.fh;
    fx = sx - 0.5f; fy = sy - 0.5f;
    return fx > -1.0f && fx < vw.fw && fy > -1.0f && fy < vw.fh;
}

/* the history of pixel (x, y) of the current view: false = none; else s holds e_r, mu1_r, mu2_r and N_r (s.n > 0) */
RPT_HD bool tp_reproject(const TpView &vw, const TpPrev &pv, uint32_t x, uint32_t y, const float4 &a0, const float4 &a1, TpSum &s) {
    s = TpSum{f3s(0.0f), 0.0f, 0.0f, 0.0f, 0.0f};
    if (vw.has_history == 0u) return false;
    const F3 n_p = f3(a0.x, a0.y, a0.z), x_p = f3(a1.x, a1.y, a1.z);
    const uint32_t kind_p = rptm::f2u(a1.w);
    const float plane = vw.footprint * a0.w;
    if (vw.identity != 0u) {
        tp_tap(vw, pv, (int)x, (int)y, 1.0f, n_p, x_p, plane, kind_p, s);
    } else {
        float fx, fy;
        if (!tp_project(vw, x_p, kind_p, fx, fy)) return false;
        const float x0f = rptm::floorr(fx), y0f = rptm::floorr(fy);
        const float a = fx - x0f, b = fy - y0f;
        const int x0 = (int)x0f, y0 = (int)y0f;                                       /* in [-1, W - 1] x [-1, H - 1] */
        const float ia = 1.0f - a, ib = 1.0f - b;
        tp_tap(vw, pv, x0, y0, ia * ib, n_p, x_p, plane, kind_p, s);
        tp_tap(vw, pv, x0 + 1, y0, a * ib, n_p, x_p, plane, kind_p, s);
        tp_tap(vw, pv, x0, y0 + 1, ia * b, n_p, x_p, plane, kind_p, s);
        tp_tap(vw, pv, x0 + 1, y0 + 1, a * b, n_p, x_p, plane, kind_p, s);
    }
    if (!(s.wt > 0.01f)) return false;
    s.e = f3(s.e.x / s.wt, s.e.y / s.wt, s.e.z / s.wt);
    s.mu1 = s.mu1 / s.wt;
    s.mu2 = s.mu2 / s.wt;
    const float n = s.n / s.wt;
    s.n = n > vw.max_history ? vw.max_history : n;
    return s.n > 0.0f;
}

/* what a pixel hands on: (e | v) to the passes, T to the caller, (e | N), (mu1, mu2) to the next view */
struct TpOut { F3 e; float v, T, N, mu1, mu2; bool reused; };

/* One pixel: e_cur = the current mean in the filter's units (demodulated already where `demodulated`), m = its moments record, a0 / a1 = its guide records. */
RPT_HD TpOut tp_pixel(const TpView &vw, const TpPrev &pv, uint32_t x, uint32_t y, F3 e_cur, const float4 &m, const float4 &a0, const float4 &a1, bool demodulated, F3 albedo) {
    TpOut o;
    const float n_cur = m.z;
    TpSum s;
    o.reused = dn_finite3(e_cur) && tp_reproject(vw, pv, x, y, a0, a1, s);
    if (!o.reused) {
        o.e = e_cur;
        o.v = dn_prepare_variance(m, demodulated, albedo);
        o.mu1 = m.x / n_cur;
        o.mu2 = m.y / n_cur;
        o.T = n_cur;
    } else {
        const float T = s.n + n_cur;
        o.e = f3((s.n * s.e.x + n_cur * e_cur.x) / T, (s.n * s.e.y + n_cur * e_cur.y) / T, (s.n * s.e.z + n_cur * e_cur.z) / T);
        const bool sums = rptm::finiter(m.x) && rptm::finiter(m.y);
        o.mu1 = (s.n * s.mu1 + (sums ? m.x : 0.0f)) / T;
        o.mu2 = (s.n * s.mu2 + (sums ? m.y : 0.0f)) / T;
        o.T = T;
        o.v = rptm::u2f(0x7f800000u);
        if (T >= 2.0f && rptm::finiter(o.mu1) && rptm::finiter(o.mu2)) {
            const float ss = o.mu2 - o.mu1 * o.mu1;
            o.v = (ss > 0.0f ? ss : 0.0f) / (T - 1.0f);
            if (demodulated && mo_variance_known(o.v)) {
                const F3 a = dn_albedo_floor(albedo);
                const float Ya = mo_luminance(a.x, a.y, a.z);
                o.v = o.v / (Ya * Ya);
            }
        }
    }
    o.N = dn_finite3(o.e) ? o.T : 0.0f;
    return o;
}

/* The fused kernel: prepare (the mean of k_dn_prepare_var, OWN: every pixel by its own .w), reproject, blend, history write.  The mapping of k_dn_pass — a
 * wave is a 64 x 1 row segment, a workgroup 64 x 4 pixels — so that the history taps of a wave are (nearly) a row segment of the previous view; `inverse`
 * != null: the accumulator and (unless moments_row_major) the moments are tile-major and inverse[at] is the element of row-major pixel `at`.
 * No LDS, no scratch.  *with_history += the pixels that reused history: one ballot and one integer atomic per wave (the order does not matter). */
template <bool OWN>
__global__ __launch_bounds__(256) void k_dn_temporal(TpView vw, TpPrev pv, const float4 *sums, const float4 *moments, const uint32_t *inverse, uint32_t moments_row_major, float sample_count,
                                                     const float4 *g0, const float4 *g1, const float4 *albedo /* null: no demodulation */, float4 *out, float4 *h_out, float2 *mu_out, float *t_out,
                                                     unsigned long long *with_history) {
    const uint32_t x = blockIdx.x * 64u + (threadIdx.x & 63u), y = blockIdx.y * 4u + (threadIdx.x >> 6);
    bool reused = false;
    if (x < vw.width && y < vw.height) {
        const size_t at = (size_t)y * vw.width + x;
        const size_t i = inverse ? (size_t)inverse[at] : at;
        const float4 a = sums[i];
        F3 c = OWN ? mean_own(a) : f3(a.x / sample_count, a.y / sample_count, a.z / sample_count);
        F3 al = f3s(1.0f);
        if (albedo) { al = xyz4(albedo[at]); c = dn_demodulate(c, al); }
        const TpOut o = tp_pixel(vw, pv, x, y, c, moments[moments_row_major ? at : i], g0[at], g1[at], albedo != nullptr, al);
        out[at] = make_float4(o.e.x, o.e.y, o.e.z, o.v);
        h_out[at] = make_float4(o.e.x, o.e.y, o.e.z, o.N);
        mu_out[at] = make_float2(o.mu1, o.mu2);
        t_out[at] = o.T;
        reused = o.reused;
    }
    const unsigned long long mask = rpt_ballot(reused);
    if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(with_history, (unsigned long long)__popcll(mask));
}

#endif /* RPT_K_TEMPORAL_H */
