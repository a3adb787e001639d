"""numpy restatement of csrc/k_adaptive.h — the selection rule of rpt_render_adaptive, the ordered compaction and the pass schedule — and what a context must
hold once every pixel has received its own number of samples, from tests/moments_ref.py SampleBank alone: for a count image N[y, x] the accumulator is the
in-order f32 sum of the pixel's first N samples with .w = N, the rng is seed.n + N, the moments are the restatement over the same samples.
Shared by tests/test_adaptive.py, tests/test_gpu_adaptive.py and tools/adaptive_probe.py."""
import numpy as np

import moments_ref as ref

F = np.float32


def select(m, threshold, batch_samples, max_samples):
    """adaptive_selected of every record of m (..., 4): not (noise_rel <= threshold), and the batch still fits under the cap (f32, as the header)"""
    m = np.asarray(m, F)
    with np.errstate(all="ignore"):
        return ~(ref.noise_rel(m) <= F(threshold)) & (m[..., 2] + F(batch_samples) <= F(max_samples))


def compact(flags):
    """the flagged records' flat indices in ascending order: the index list of a masked pass"""
    return np.flatnonzero(np.asarray(flags).reshape(-1)).astype(np.uint32)


def schedule(min_samples, batch_samples, max_samples):
    """the counts a pixel can stop at: min_samples, min_samples + batch_samples, ... while <= max_samples"""
    return list(range(min_samples, max_samples + 1, batch_samples))


class Target:
    def __init__(self, threshold, max_above=0, batch_samples=8, min_samples=8, max_samples=64):
        self.threshold, self.max_above, self.batch_samples, self.min_samples, self.max_samples = threshold, max_above, batch_samples, min_samples, max_samples

    def kwargs(self):
        return dict(threshold=self.threshold, max_above=self.max_above, batch_samples=self.batch_samples, min_samples=self.min_samples, max_samples=self.max_samples)


def moments_at(bank, counts, cache=None):
    """the moments record of every pixel after its own counts[y, x] samples"""
    cache = {} if cache is None else cache
    out = np.zeros(counts.shape + (4,), F)
    for n in np.unique(counts):
        n = int(n)
        if n not in cache:
            cache[n] = bank.moments(n)
        out[counts == n] = cache[n][counts == n]
    return out


def simulate(bank, t, own=None):
    """rpt_render_adaptive pass by pass, on a fresh moments record: the uniform phase, then select / count / render until converged or nothing is selected.
    own: the pixels that take part (a rank's; None = all).  Returns {"counts_image", "passes", "converged", "counts", "pixel_samples"}; pixels outside `own`
    keep count 0."""
    h, w = bank.cfg.height, bank.cfg.width
    own = np.ones((h, w), bool) if own is None else own
    n = np.where(own, t.min_samples, 0).astype(np.int64)
    cache, passes, converged = {}, 0, 0
    pixel_samples = int(own.sum()) * t.min_samples
    while True:
        m = moments_at(bank, n, cache)
        counts = ref.noise_counts(m[own], t.threshold)
        if counts["measured"] == counts["pixels"] and counts["above"] <= t.max_above:
            converged = 1
            break
        chosen = select(m, t.threshold, t.batch_samples, t.max_samples) & own
        if not chosen.any():
            break
        n[chosen] += t.batch_samples
        passes += 1
        pixel_samples += int(chosen.sum()) * t.batch_samples
    return {"counts_image": n, "passes": passes, "converged": converged, "counts": counts, "pixel_samples": pixel_samples}


def closed_form(bank, t):
    """every pixel's final count under max_above = 0: the first count of the schedule at which its noise was at or below the threshold, else the last one"""
    steps = schedule(t.min_samples, t.batch_samples, t.max_samples)
    n = np.full(bank.moments(steps[0]).shape[:2], steps[-1], np.int64)
    stopped = np.zeros(n.shape, bool)
    for k in steps:
        with np.errstate(all="ignore"):
            below = ref.noise_rel(bank.moments(k)) <= F(t.threshold)
        n[below & ~stopped] = k
        stopped |= below
    return n


def uniform_stop(bank, t):
    """rpt_render_to_noise on the same target: (samples every pixel gets, converged)"""
    n = 0
    while n < t.max_samples:
        n += min(t.batch_samples, t.max_samples - n)
        if n < t.min_samples:
            continue
        counts = ref.noise_counts(bank.moments(n), t.threshold)
        if counts["measured"] == counts["pixels"] and counts["above"] <= t.max_above:
            return n, 1
    return n, 0


def expected_state(bank, counts):
    """(accumulator, rng, moments) after every pixel received its first counts[y, x] samples, in order"""
    counts = np.asarray(counts, np.int64)
    top = int(counts.max()) if counts.size else 0
    bank.need(top)
    acc, mom = np.zeros(counts.shape + (4,), F), np.zeros(counts.shape + (4,), F)
    for k in range(top):
        live = counts > k
        acc[live, :3] = acc[live, :3] + bank.radiance[k][live]
        acc[live, 3] = acc[live, 3] + F(1)
        mom[live] = ref.add_sample(mom[live], bank.radiance[k][live])
    rng = np.ascontiguousarray(bank.rngs[0]).copy().reshape(counts.shape)
    rng["n"] = (rng["n"].astype(np.int64) + counts).astype(np.uint32)
    return acc, rng, mom

