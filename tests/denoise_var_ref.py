"""numpy restatement, in f32 and in the same operation order, of the variance-guided filter of csrc/k_denoise.h (dn_prepare_variance, dn_prefilter_variance,
dn_filter_pixel_var) and of the variance of the mean of csrc/k_moments.h (mo_variance_of_mean, mo_add).

Not a test module (no test_ prefix): tests/test_denoise_variance.py holds the host build against it.  As in tests/denoise_ref.py the exponential is the
oracle's (oracle.math(3, .), the rptm::expr the filter calls) and the display operators are oracle.resolve; everything else is plain IEEE f32 arithmetic,
which numpy performs operation by operation without fusing.  Also here: the inputs of the quality comparison — the oracle images of
denoise_ref.quality_images together with the moments record of the noisy image's samples.
"""
import functools

import numpy as np

import denoise_ref
from denoise_ref import F, H5, KIND_MISS, albedo_floor, dot3, finite3

INF = F(np.inf)
G3 = {-1: F(0.25), 0: F(0.5), 1: F(0.25)}


def luminance(c):
    """mo_luminance over the last axis"""
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def moments_add(m, rgb):
    """mo_add: one sample of radiance rgb (..., 3) into the records m (..., 4), in place"""
    y = luminance(rgb).astype(F)
    yy = (y * y).astype(F)
    m[..., 0] = m[..., 0] + y
    m[..., 1] = m[..., 1] + yy
    m[..., 2] = m[..., 2] + F(1.0)
    m[..., 3] = np.where(y > m[..., 3], y, m[..., 3])
    return m


def variance_of_mean(m):
    """mo_variance_of_mean: +inf = unknown"""
    with np.errstate(all="ignore"):
        n = m[..., 2]
        known = (n >= F(2.0)) & np.isfinite(m[..., 0]) & np.isfinite(m[..., 1])
        ss = m[..., 1] - (m[..., 0] * m[..., 0]) / n
        v = np.where(ss > F(0.0), ss, F(0.0)).astype(F) / (n * (n - F(1.0)))
    return np.where(known, v, INF).astype(F)


def known(v):
    return np.isfinite(v)


def prepare_variance(moments, demodulated, albedo):
    """dn_prepare_variance"""
    v = variance_of_mean(moments)
    if demodulated:
        ya = luminance(albedo_floor(albedo)).astype(F)
        with np.errstate(all="ignore"):
            v = np.where(known(v), v / (ya * ya), v).astype(F)
    return v


def prefilter_variance(v, kind):
    """dn_prefilter_variance for every pixel"""
    h, w = v.shape
    ys, xs = np.mgrid[0:h, 0:w]
    acc, ksum = np.zeros((h, w), F), np.zeros((h, w), F)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            k = F(G3[dx] * G3[dy])
            qy, qx = ys + dy, xs + dx
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            v_q = v[qy, qx]
            ok = inside & (kind[qy, qx] == kind) & known(v_q)
            acc = np.where(ok, acc + k * np.where(ok, v_q, F(0.0)), acc).astype(F)
            ksum = np.where(ok, ksum + k, ksum).astype(F)
    return np.where(ksum > 0, acc / np.where(ksum > 0, ksum, F(1.0)), INF).astype(F)


def filter_pass_var(e, v, normal, position, depth, kind, i, normal_power_log2, sigma_color, sigma_plane, sigma_variance, expr):
    """dn_filter_pixel_var for every pixel: pass i (step 2^i) over the (H, W, 3) image e and its (H, W) variance v; returns (e, v)"""
    h, w = e.shape[:2]
    step = 1 << i
    plane_scale = F(F(sigma_plane) * F(step)) * F(F(2.0) / F(w))
    sigma_i = F(F(sigma_color) * F(2.0 ** -i))
    sigma2 = F(sigma_i * sigma_i)
    plane = (plane_scale * depth).astype(F)
    ep2 = dot3(e, e)
    centre_ok = finite3(e)
    lum_term = np.zeros((h, w), bool)
    if sigma_variance != 0.0:
        vbar = prefilter_variance(v, kind)
        lum_term = known(vbar)
        lum_width = (F(sigma_variance) * np.sqrt(np.where(lum_term, vbar, F(0.0))) + F(1e-6)).astype(F)
        y_p = luminance(e).astype(F)
    total = np.zeros_like(e)
    wsum, vsum = np.zeros((h, w), F), np.zeros((h, w), F)
    joined = np.zeros((h, w), bool)
    ys, xs = np.mgrid[0:h, 0:w]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            k = F(H5[dx] * H5[dy])
            qy, qx = ys + dy * step, xs + dx * step
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            e_q, v_q = e[qy, qx], v[qy, qx]
            if dx == 0 and dy == 0:
                wt = np.full((h, w), k, F)
                ok = inside
            else:
                ok = inside & (kind[qy, qx] == kind) & finite3(e_q)
                hit = kind != KIND_MISS
                ndot = dot3(normal, normal[qy, qx])
                w_n = np.where(F(0.0) > ndot, F(0.0), np.where(np.isnan(ndot), F(0.0), ndot)).astype(F)      # fmaxr(0, n_p . n_q)
                for _ in range(normal_power_log2):
                    w_n = w_n * w_n
                w_n = np.where(hit, w_n, F(1.0)).astype(F)
                d = np.abs(dot3(normal, position[qy, qx] - position)) / plane
                d = np.where(hit, d, F(0.0)).astype(F)
                if sigma2 != 0.0:
                    diff = e - e_q
                    d = d + dot3(diff, diff) / (sigma2 * ((ep2 + dot3(e_q, e_q)) + F(1e-12)))
                if sigma_variance != 0.0:
                    d = np.where(lum_term, d + np.abs(y_p - luminance(e_q)) / lum_width, d).astype(F)
                wt = (k * w_n) * expr((-d).astype(F))
                ok = ok & (wt > 0.0)
                joined |= ok
            total = np.where(ok[..., None], total + wt[..., None] * e_q, total)
            wsum = np.where(ok, wsum + wt, wsum)
            okv = ok & known(v_q)
            vsum = np.where(okv, vsum + (wt * wt) * np.where(okv, v_q, F(0.0)), vsum).astype(F)
    out = total / wsum[..., None]
    v_out = np.where(known(v), vsum / (wsum * wsum), INF).astype(F)
    through = centre_ok & joined
    return np.where(through[..., None], out, e).astype(F), np.where(through, v_out, v).astype(F)


def denoise_variance(mean, guides, moments, params, tonemap_op, oracle):
    """rpt_denoise_variance / rpt_debug_denoise_variance_host: mean (H, W, 3), guides as Renderer.guides() returns them, moments (H, W, 4), params with the
    fields of rpt_denoise_var_params; returns (rgb, variance)"""
    expr = lambda x: oracle.math(3, np.ascontiguousarray(x, F))
    mean, moments = np.ascontiguousarray(mean, F), np.ascontiguousarray(moments, F)
    albedo = np.ascontiguousarray(guides["albedo"], F)
    normal, position = np.ascontiguousarray(guides["normal"], F), np.ascontiguousarray(guides["position"], F)
    depth, kind = np.ascontiguousarray(guides["depth"], F), np.ascontiguousarray(guides["kind"], np.uint32)
    b = params.base
    demodulated = b.iterations != 0 and b.demodulate != 0
    with np.errstate(all="ignore"):
        e = (mean / albedo_floor(albedo)).astype(F) if demodulated else mean
        v = prepare_variance(moments, demodulated, albedo)
        for i in range(b.iterations):
            e, v = filter_pass_var(e, v, normal, position, depth, kind, i, b.normal_power_log2, b.sigma_color, b.sigma_plane, params.sigma_variance, expr)
        if demodulated:
            e = (e * albedo_floor(albedo)).astype(F)
    return denoise_ref.tonemap(e, tonemap_op, oracle), v


# ---- quality ---------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _quality_inputs(rpt, world, oracle, scene, nee, noisy_spp, converged_spp):
    W = H = 128
    cfg = rpt.default_config(W, H, nee=nee)
    w = world(scene)
    sc = oracle.scene(w)
    rng = rpt.blue_noise_seeds(W, H)
    moments, noisy = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
    for _ in range(noisy_spp):                                           # one sample at a time into a zero accumulator: 0 + s = s, the sample itself
        s, rng, _ = oracle.trace_cpu(cfg, sc, rng, 1)
        moments_add(moments, s[..., :3])
        noisy = (noisy + s).astype(F)                                    # the accumulator's own order of additions
    conv, _, _ = oracle.trace_cpu(cfg, sc, rng, converged_spp - noisy_spp, accum=noisy)
    return ((noisy[..., :3] / F(noisy_spp)).astype(F), (conv[..., :3] / F(converged_spp)).astype(F), denoise_ref.guides(w, cfg, oracle, sc), moments, noisy)


def quality_inputs(rpt, world, oracle, scene, nee, noisy_spp=8, converged_spp=1024):
    """denoise_ref.quality_images (the same oracle images, bit for bit: test_denoise_variance.py checks the noisy one) and the moments record of the noisy
    image's samples: (noisy mean, converged mean, guides, moments (H, W, 4), noisy sums (H, W, 4)).  Computed once per process and scene; treat as read-only."""
    return _quality_inputs(rpt, world, oracle, scene, nee, noisy_spp, converged_spp)
