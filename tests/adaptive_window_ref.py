"""numpy restatement of the window rule of rpt_render_adaptive_window (csrc/k_adaptive.h k_ad_window; include/rpt/rpt.h "adaptive sampling by a pixel's
NEIGHBOURHOOD"): a pixel is selected while any pixel within `radius` of it, inside the image and inside its own 64 x 64 tile, is above the threshold, and the
batch still fits under its cap.  The dilation here is a sum of shifted boolean images per tile — nothing of the header's row words and shifts — and the pass
schedule is tests/adaptive_ref.py simulate with that selection in place of the per-pixel one.
Shared by tests/test_adaptive_window.py, tests/test_gpu_adaptive_window.py and tools/adaptive_probe.py."""
import numpy as np

import adaptive_ref as aref
import moments_ref as ref

F = np.float32
TILE = 64
MAX_RADIUS = 8


def above(m, threshold):
    """not (noise_rel <= threshold): an unmeasured record, +inf and a NaN are above"""
    with np.errstate(all="ignore"):
        return ~(ref.noise_rel(np.asarray(m, F)) <= F(threshold))


def fits(m, batch_samples, max_samples):
    m = np.asarray(m, F)
    with np.errstate(all="ignore"):
        return m[..., 2] + F(batch_samples) <= F(max_samples)


def dilate_tiles(a, radius):
    """every pixel of the (H, W) boolean image a: is any pixel within `radius` in x and in y, inside the pixel's own tile, set"""
    a = np.asarray(a, bool)
    out = np.zeros_like(a)
    for ty in range(0, a.shape[0], TILE):
        for tx in range(0, a.shape[1], TILE):
            t = a[ty:ty + TILE, tx:tx + TILE]
            h, w = t.shape
            padded = np.zeros((h + 2 * radius, w + 2 * radius), bool)
            padded[radius:radius + h, radius:radius + w] = t
            near = np.zeros((h, w), bool)
            for dy in range(2 * radius + 1):
                for dx in range(2 * radius + 1):
                    near |= padded[dy:dy + h, dx:dx + w]
            out[ty:ty + TILE, tx:tx + TILE] = near
    return out


def select(m, threshold, batch_samples, max_samples, radius):
    """selected(p) of every record of the row-major image m (H, W, 4)"""
    return dilate_tiles(above(m, threshold), radius) & fits(m, batch_samples, max_samples)


def owned(width, height, rank, world):
    """(H, W) bool: the pixels of the tiles with id mod world == rank"""
    yy, xx = np.mgrid[0:height, 0:width]
    return ((yy // TILE) * ((width + TILE - 1) // TILE) + xx // TILE) % world == rank


def simulate(bank, t, radius, own=None):
    """rpt_render_adaptive_window pass by pass, as adaptive_ref.simulate: the counts are about each pixel's OWN noise, the selection is the window rule.
    Adds "first_mask" (the selection before the first masked pass, None if there was none) and "selected_per_pass"."""
    h, w = bank.cfg.height, bank.cfg.width
    own = np.ones((h, w), bool) if own is None else own
    n = np.where(own, t.min_samples, 0).astype(np.int64)
    cache, passes, converged, first, per_pass = {}, 0, 0, None, []
    pixel_samples = int(own.sum()) * t.min_samples
    while True:
        m = aref.moments_at(bank, n, cache)
        counts = ref.noise_counts(m[own], t.threshold)
        if counts["measured"] == counts["pixels"] and counts["above"] <= t.max_above:
            converged = 1
            break
        chosen = select(m, t.threshold, t.batch_samples, t.max_samples, radius) & own
        if first is None:
            first = chosen.copy()
        if not chosen.any():
            break
        n[chosen] += t.batch_samples
        passes += 1
        per_pass.append(int(chosen.sum()))
        pixel_samples += int(chosen.sum()) * t.batch_samples
    return {"counts_image": n, "passes": passes, "converged": converged, "counts": counts, "pixel_samples": pixel_samples, "first_mask": first,
            "selected_per_pass": per_pass}
