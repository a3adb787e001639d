"""numpy restatement, in f32 and in the same operation order, of the firefly clamp of csrc/k_firefly.h (ff_pixel), an independent float64 restatement of
the same rule, and the whole calls: the clamp composed with tests/denoise_var_ref.py and tests/temporal_ref.py, which are imported and not edited.

Not a test module (no test_ prefix): tests/test_denoise_firefly.py holds the host build against it, tests/test_gpu_denoise_firefly.py the device.
"""
import numpy as np

import denoise_var_ref
import temporal_ref
from denoise_ref import F, albedo_floor

D = np.float64


def window_max(moments, kind, ya, radius, dtype=F):
    """(any eligible tap, B): the largest b(q) = m_q.w / Ya_q over the eligible taps of every pixel's window, dy outer, dx inner, both ascending"""
    h, w = kind.shape
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        b = (moments[..., 3].astype(dtype) / ya).astype(dtype)
    tap_ok = (moments[..., 2] >= 1) & np.isfinite(b)
    has, big = np.zeros((h, w), bool), np.zeros((h, w), dtype)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dx == 0 and dy == 0:
                continue
            qy, qx = ys + dy, xs + dx
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            ok = inside & (kind[qy, qx] == kind) & tap_ok[qy, qx]
            b_q = b[qy, qx]
            take = ok & (~has | (b_q > big))
            big = np.where(take, b_q, big).astype(dtype)
            has |= ok
    return has, big


def limit(albedo, kind, moments, scale, floor, radius, demodulated):
    """(any eligible tap, L) of every pixel in f32: L = max(scale * B, floor) * Ya_p"""
    moments, kind = np.ascontiguousarray(moments, F), np.ascontiguousarray(kind, np.uint32)
    h, w = kind.shape
    ya = denoise_var_ref.luminance(albedo_floor(np.ascontiguousarray(albedo, F))).astype(F) if demodulated else np.ones((h, w), F)
    with np.errstate(all="ignore"):
        has, big = window_max(moments, kind, ya, radius)
        sb = (F(scale) * big).astype(F)
        return has, (np.where(sb > F(floor), sb, F(floor)).astype(F) * ya).astype(F)


def clamp(mean, albedo, kind, moments, counts, scale, floor, radius, demodulated):
    """ff_pixel for every pixel, f32: mean (H, W, 3) in radiance units, counts (H, W) or a scalar; returns (c', m', mask)"""
    mean, moments = np.ascontiguousarray(mean, F), np.ascontiguousarray(moments, F)
    kind = np.ascontiguousarray(kind, np.uint32)
    h, w = kind.shape
    counts = np.broadcast_to(np.asarray(counts, F), (h, w))
    has, L = limit(albedo, kind, moments, scale, floor, radius, demodulated)
    with np.errstate(all="ignore"):
        mx, my, n, wmax = (moments[..., k] for k in range(4))
        mask = has & (n >= F(1.0)) & (n == counts) & np.isfinite(mx) & np.isfinite(my) & np.isfinite(wmax) & np.isfinite(L) & (mx > F(0.0)) & (wmax > L)
        x1 = ((mx - wmax).astype(F) + L).astype(F)
        x1 = np.where(x1 < F(0.0), F(0.0), x1).astype(F)
        y1 = ((my - (wmax * wmax).astype(F)).astype(F) + (L * L).astype(F)).astype(F)
        y1 = np.where(y1 < F(0.0), F(0.0), y1).astype(F)
        rho = (x1 / mx).astype(F)
        rho = np.where(rho > F(1.0), F(1.0), rho).astype(F)
        c1 = (mean * rho[..., None]).astype(F)
    out_c = np.where(mask[..., None], c1, mean).astype(F)
    out_m = np.where(mask[..., None], np.stack([x1, y1, n, L], -1), moments).astype(F)
    return out_c, out_m, mask


def clamp64(mean, albedo, kind, moments, counts, scale, floor, radius, demodulated):
    """The rule in float64, written from the rule's text and not from clamp(): per pixel the window's largest eligible b, the limit, the decision, the clamped
    sums.  Returns a dictionary: has, B, L, w (the brightest sample), mask, eligible (H, W) of the pixel as a TAP, x1, y1, rho, c1 (unmasked values)."""
    mean, moments, albedo = np.asarray(mean, D), np.asarray(moments, D), np.asarray(albedo, D)
    kind = np.asarray(kind)
    h, w = kind.shape
    counts = np.broadcast_to(np.asarray(counts, D), (h, w))
    if demodulated:
        a = np.maximum(albedo, D(F(0.01)))
        ya = D(F(0.2126)) * a[..., 0] + D(F(0.7152)) * a[..., 1] + D(F(0.0722)) * a[..., 2]
    else:
        ya = np.ones((h, w), D)
    with np.errstate(all="ignore"):
        b = moments[..., 3] / ya
        # (a b that is finite in float64 but overflows f32 is an infinity to the f32 rule: decided as f32 decides it, such a case is not a rounding question)
        eligible = (moments[..., 2] >= 1) & np.isfinite(b) & (np.abs(b) <= D(np.finfo(F).max))
        big = np.full((h, w), -np.inf, D)
        has = np.zeros((h, w), bool)
        for y in range(h):
            for x in range(w):
                y0, y1_, x0, x1_ = max(0, y - radius), min(h, y + radius + 1), max(0, x - radius), min(w, x + radius + 1)
                ok = eligible[y0:y1_, x0:x1_] & (kind[y0:y1_, x0:x1_] == kind[y, x])
                ok[y - y0, x - x0] = False
                if ok.any():
                    has[y, x] = True
                    big[y, x] = b[y0:y1_, x0:x1_][ok].max()
        L = np.maximum(D(F(scale)) * np.where(has, big, 0.0), D(F(floor))) * ya
        mx, my, n, wmax = (moments[..., k] for k in range(4))
        fin = np.isfinite(mx) & np.isfinite(my) & np.isfinite(wmax) & np.isfinite(L) & (np.abs(L) <= D(np.finfo(F).max))
        mask = has & (n >= 1) & (n == counts) & fin & (mx > 0) & (wmax > L)
        x1 = np.maximum((mx - wmax) + L, 0.0)
        y1 = np.maximum((my - wmax * wmax) + L * L, 0.0)
        rho = np.minimum(x1 / mx, 1.0)
        c1 = mean * rho[..., None]
    return {"has": has, "B": big, "L": L, "w": wmax, "mask": mask, "eligible": eligible, "x1": x1, "y1": y1, "rho": rho, "c1": c1}


def denoise_variance(mean, guides, moments, params, tonemap_op, oracle, counts=None):
    """rpt_denoise_variance with the clamp: clamp(), then tests/denoise_var_ref.py on (c', m').  counts None: the record's own m.z, as the host hook takes it.
    Returns (rgb, variance, mask)."""
    b = params.base
    demodulated = b.iterations != 0 and b.demodulate != 0
    moments = np.ascontiguousarray(moments, F)
    mask = np.zeros(moments.shape[:2], bool)
    if params.clamp_scale != 0.0:
        mean, moments, mask = clamp(mean, guides["albedo"], guides["kind"], moments, moments[..., 2] if counts is None else counts, params.clamp_scale, params.clamp_floor,
                                    params.clamp_radius, demodulated)
    return denoise_var_ref.denoise_variance(mean, guides, moments, params, tonemap_op, oracle) + (mask,)


def denoise_temporal(mean, guides, moments, camera, previous, params, tonemap_op, oracle, counts=None):
    """rpt_denoise_temporal with the clamp: clamp(), then tests/temporal_ref.py on (c', m'); the dictionary of temporal_ref.denoise_temporal and "mask" """
    b = params.filter.base
    demodulated = b.iterations != 0 and b.demodulate != 0
    moments = np.ascontiguousarray(moments, F)
    mask = np.zeros(moments.shape[:2], bool)
    f = params.filter
    if f.clamp_scale != 0.0:
        mean, moments, mask = clamp(mean, guides["albedo"], guides["kind"], moments, moments[..., 2] if counts is None else counts, f.clamp_scale, f.clamp_floor, f.clamp_radius,
                                    demodulated)
    out = temporal_ref.denoise_temporal(mean, guides, moments, camera, previous, params, tonemap_op, oracle)
    out["mask"] = mask
    return out
