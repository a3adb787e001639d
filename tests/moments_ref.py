"""numpy restatement of csrc/k_moments.h — the per-pixel moments record and noise_rel, f32 operation by f32 operation in the header's order — and the
per-sample radiances it is fed with, taken from the CPU oracle alone: one-sample calls of oracle.trace_cpu chained through the returned rng give every
sample's radiance exactly (their in-order f32 sum is the oracle's n-sample accumulator bit for bit, which SampleBank.accum is checked against where it
is used).  Shared by tests/test_moments.py, tests/test_gpu_moments.py and tools/moments_probe.py."""
import numpy as np

F = np.float32
WR, WG, WB = F(0.2126), F(0.7152), F(0.0722)
STAT_KEYS = ("extension_rays", "shadow_rays", "sky_evals")


def luminance(r):
    return (WR * r[..., 0] + WG * r[..., 1]) + WB * r[..., 2]


def add_sample(m, r):
    """mo_add: one sample of radiance r (..., 3) into the records m (..., 4), in place"""
    y = luminance(r)
    with np.errstate(all="ignore"):
        m[..., 0] = m[..., 0] + y
        m[..., 1] = m[..., 1] + y * y
        m[..., 2] = m[..., 2] + F(1)
        m[..., 3] = np.where(y > m[..., 3], y, m[..., 3])
    return m


def noise_rel(m):
    """noise_rel of every record of m (..., 4) float32"""
    m = np.asarray(m, F)
    sx, sy, n = m[..., 0], m[..., 1], m[..., 2]
    with np.errstate(all="ignore"):
        mean = sx / n
        ss = sy - (sx * sx) / n
        v = ss / (n * (n - F(1)))
        sem = np.sqrt(np.where(v > 0, v, F(0)))
        rel = sem / (np.abs(mean) + F(0.01))
    return np.where((n >= 2) & np.isfinite(sx) & np.isfinite(sy), rel, F(np.inf)).astype(F)


def noise_counts(m, threshold):
    m = np.asarray(m, F).reshape(-1, 4)
    measured = m[:, 2] >= 2
    with np.errstate(all="ignore"):
        above = measured & ~(noise_rel(m) <= F(threshold))
    return {"pixels": len(m), "measured": int(measured.sum()), "above": int(above.sum())}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


class SampleBank:
    """every sample's radiance of one (scene, config, seeds), from the oracle, computed once and extended on demand"""

    def __init__(self, oracle, cfg, world, seeds, skybox_f32=None):
        self.oracle, self.cfg, self.scene = oracle, cfg, oracle.scene(world, skybox_f32=skybox_f32)
        self.rngs = [np.ascontiguousarray(seeds).copy()]        # rngs[k]: the state after k samples
        self.radiance, self.stats = [], []

    def need(self, n):
        while len(self.radiance) < n:
            acc, rng, st = self.oracle.trace_cpu(self.cfg, self.scene, self.rngs[-1], 1)
            self.radiance.append(acc[..., :3].copy())
            self.rngs.append(rng)
            self.stats.append({k: getattr(st, k) for k in STAT_KEYS})

    def rng(self, n):
        self.need(n)
        return self.rngs[n]

    def accum(self, n, first=0):
        """the accumulator after the samples first .. n - 1 were added to zeros, in order: (H, W, 4)"""
        self.need(n)
        acc = np.zeros(self.radiance[0].shape[:2] + (4,), F)
        for k in range(first, n):
            acc[..., :3] = acc[..., :3] + self.radiance[k]
            acc[..., 3] = acc[..., 3] + F(1)
        return acc

    def moments(self, n, first=0):
        """the moments record after the samples first .. n - 1, started from zeros"""
        self.need(n)
        m = np.zeros(self.radiance[0].shape[:2] + (4,), F)
        for k in range(first, n):
            add_sample(m, self.radiance[k])
        return m

    def ray_counts(self, n):
        self.need(n)
        return {k: sum(s[k] for s in self.stats[:n]) for k in STAT_KEYS}
