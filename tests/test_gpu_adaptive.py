"""GPU tests of rendering chosen pixels (rpt_render_pixels, rpt_render_adaptive, rpt_counts_uniform and their rpt_multi_* forms; csrc/k_adaptive.h,
rpt_adaptive.hip).

The contract: a pixel that has received N samples by any route holds, bit for bit, what the CPU oracle holds after N samples.  So every case compares
accumulator, rng and moments word for word with tests/adaptive_ref.py expected_state — the in-order f32 sum of each pixel's first N[y, x] samples from
tests/moments_ref.py SampleBank, rng = seed.n + N, the moments restated over the same samples — and rpt_stats.samples with the pixel-samples rendered.
Images are 100 x 70 with nee 1 (7 000 pixels: the last chunk of 64 is padded); DarkCornell is walked from LDS, VeachMIS from global memory."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as aref
import moments_ref as ref

pytestmark = pytest.mark.gpu

W0, H0 = 100, 70
F = np.float32
_banks = {}


def bank(oracle, rpt, world, scene):
    """the per-sample radiances of (scene, nee 1, 100 x 70, blue-noise seeds): computed once for the session, extended on demand, never changed"""
    if scene not in _banks:
        _banks[scene] = ref.SampleBank(oracle, rpt.default_config(W0, H0, nee=1), world(scene), rpt.blue_noise_seeds(W0, H0))
    return _banks[scene]


class fresh:
    """a Renderer of its own with the scene and configuration of a bank, reset to its seeds"""

    def __init__(self, hipmod, world, scene, b, moments=True, in_flight=None, partition=None, reset=True):
        self.r = hipmod.Renderer(0) if partition is None else hipmod.Renderer(0, *partition)
        try:
            if in_flight is not None:
                self.r.set_samples_in_flight(in_flight)
            self.r.upload_scene(world(scene))
            self.r.set_config(b.cfg)
            if reset:
                self.r.reset(b.rng(0))
            if moments:
                self.r.set_moments(True)
        except Exception:
            self.r.close()
            raise

    def __enter__(self):
        return self.r

    def __exit__(self, *exc):
        self.r.close()


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def tile_positions(hipmod, rank=0, world_size=1):
    """(y, x) of the rank's pixels in its tile-major pixel order"""
    xy = hipmod.tile_order(W0, H0, rank, world_size)
    return (xy >> 16).astype(np.int64), (xy & 0xFFFF).astype(np.int64)


def first_in_tile_order(hipmod, n):
    y, x = tile_positions(hipmod)
    m = np.zeros((H0, W0), bool)
    m[y[:n], x[:n]] = True
    return m


def straddling(hipmod):
    """257 pixels of the pixel order: two runs across the boundaries of the compaction's workgroups of 256 pixels (250 .. 261, 506 .. 517) and every 30th"""
    idx = sorted(set(range(250, 262)) | set(range(506, 518)) | set(range(0, W0 * H0, 30)))
    assert len(idx) == 257
    y, x = tile_positions(hipmod)
    m = np.zeros((H0, W0), bool)
    m[y[idx], x[idx]] = True
    return m


def checkerboard():
    yy, xx = np.mgrid[0:H0, 0:W0]
    return (yy + xx) % 2 == 0


def single(x, y):
    m = np.zeros((H0, W0), bool)
    m[y, x] = True
    return m


def masks(hipmod):
    return {"empty": np.zeros((H0, W0), bool), "all": np.ones((H0, W0), bool), "pixel (0, 0)": single(0, 0), "pixel (99, 69)": single(99, 69),
            "first 63": first_in_tile_order(hipmod, 63), "first 64": first_in_tile_order(hipmod, 64), "first 65": first_in_tile_order(hipmod, 65),
            "257 straddling": straddling(hipmod), "checkerboard": checkerboard()}


def check_counts(r, b, counts, own=None, moments=True, rendered=None, what=""):
    """accumulator, rng and moments of the renderer == the reference for the count image, word for word (own: the rank's pixels, all others zero);
    rendered: the pixel-samples rpt_stats.samples must report"""
    own = np.ones((H0, W0), bool) if own is None else own
    want_acc, want_rng, want_mom = aref.expected_state(b, np.where(own, counts, 0))
    acc, _ = r.read_accum()
    rng = r.read_rng().reshape(H0, W0)
    bad = int((acc.view(np.uint32) != want_acc.view(np.uint32)).any(axis=-1).sum())
    print(f"{what}: {int(np.where(own, counts, 0).sum())} pixel-samples, {bad} accumulator pixels differ")
    assert bad == 0, what
    assert np.array_equal(rng[own], want_rng[own]) and not rng[~own].view(np.uint32).any(), what
    if moments:
        assert same_words(r.read_moments(), want_mom), what
    if rendered is not None:
        assert r.stats()["samples"] == rendered, what
    return acc


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "plain"])
@pytest.mark.parametrize("n", [1, 5, 40])
@pytest.mark.parametrize("scene", ["DarkCornell", "VeachMIS"])
def test_masks(hipmod, oracle, rpt, world, scene, n, moments):
    """every mask from a fresh reset: the selected pixels hold n samples, the others nothing"""
    b = bank(oracle, rpt, world, scene)
    with fresh(hipmod, world, scene, b, moments=moments) as r:
        for name, mask in masks(hipmod).items():
            r.reset(b.rng(0))
            r.render_pixels(mask, n)
            what = f"{scene}, {name}, n = {n}"
            acc = check_counts(r, b, mask * n, moments=moments, rendered=int(mask.sum()) * n, what=what)
            samples = r.read_accum()[1]
            if name == "all":                                 # the uniform call it amounts to: rpt_render's image, counts and sample count
                st = r.stats()
                assert samples == n and r.counts_uniform() and {k: st[k] for k in ref.STAT_KEYS} == b.ray_counts(n), what
                r.reset(b.rng(0))
                r.render(n)
                assert r.read_accum()[0].tobytes() == acc.tobytes(), what
            else:
                assert samples == 0 and r.counts_uniform() == (name == "empty"), what


def test_polled_path(hipmod, oracle, rpt, world):
    """4 slots per pixel, 9 samples under a checkerboard: the slots of the view take several samples, the completion runs after every shade stage"""
    for scene in ("DarkCornell", "VeachMIS"):
        b = bank(oracle, rpt, world, scene)
        with fresh(hipmod, world, scene, b, in_flight=4) as r:
            r.render_pixels(checkerboard(), 9)
            check_counts(r, b, checkerboard() * 9, rendered=3500 * 9, what=f"{scene}, polled")


def test_slot_layout_q_shift_3(monkeypatch, hipmod, oracle, rpt, world):
    monkeypatch.setenv("RPT_SLOT_Q_SHIFT", "3")
    for scene in ("DarkCornell", "VeachMIS"):
        b = bank(oracle, rpt, world, scene)
        with fresh(hipmod, world, scene, b) as r:
            r.render_pixels(checkerboard(), 16)
            check_counts(r, b, checkerboard() * 16, rendered=3500 * 16, what=f"{scene}, q_shift 3")


@pytest.mark.parametrize("scene", ["DarkCornell", "VeachMIS"])
def test_sequence_of_uniform_and_masked_calls(hipmod, oracle, rpt, world, scene):
    """uniform 8, mask A x 5, uniform 3, mask B x 16 (A and B overlap), the last two asynchronous with one wait: counts 11 / 16 / 27 / 32"""
    b = bank(oracle, rpt, world, scene)
    xx = np.mgrid[0:H0, 0:W0][1]
    A, B = xx < 50, (xx >= 30) & (xx < 80)                     # neither: x >= 80
    counts = 11 + 5 * A + 16 * B
    assert sorted(np.unique(counts)) == [11, 16, 27, 32]
    with fresh(hipmod, world, scene, b) as r:
        r.render(8)
        r.render_pixels(A, 5)
        r.render_async(3)
        r.render_pixels(B, 16)
        r.wait()
        acc = check_counts(r, b, counts, rendered=W0 * H0 * 11 + int(A.sum()) * 5 + int(B.sum()) * 16, what=f"{scene}, sequence")
        assert np.array_equal(acc[..., 3], counts.astype(F))
        assert r.read_accum()[1] == 11 and not r.counts_uniform()
        with np.errstate(all="ignore"):
            want = acc[..., :3] / acc[..., 3:4]
        assert same_words(r.resolve(0), want)                     # every pixel by its own count
        # denoise without a pass is the resolve, own counts included
        assert r.denoise(params=hipmod.denoise_params(iterations=0), tonemap_op=0).tobytes() == r.resolve(0).tobytes()
        assert r.denoise(params=hipmod.denoise_params(iterations=0), tonemap_op=4).tobytes() == r.resolve(4).tobytes()
        r.reset(b.rng(0))
        assert r.counts_uniform() and r.read_accum()[1] == 0
        r.render(5)                                               # and the context renders as it always did
        check_counts(r, b, np.full((H0, W0), 5), rendered=W0 * H0 * 5, what=f"{scene}, after reset")
        assert same_words(r.resolve(0), oracle.resolve(b.accum(5), 5.0, 0))


def test_a_pixel_without_samples_resolves_to_zero(hipmod, oracle, rpt, world):
    b = bank(oracle, rpt, world, "DarkCornell")
    with fresh(hipmod, world, "DarkCornell", b, moments=False) as r:
        r.render_pixels(checkerboard(), 5)
        rgb, acc = r.resolve(0), r.read_accum()[0]
        assert not rgb[~checkerboard()].view(np.uint32).any()
        assert same_words(rgb[checkerboard()], acc[checkerboard()][:, :3] / acc[checkerboard()][:, 3:4])
        assert r.denoise(params=hipmod.denoise_params(iterations=0)).tobytes() == rgb.tobytes()


def test_partition_and_multi_gpu(hipmod, oracle, rpt, world):
    """rank 1 of 3 owns the tile x >= 64, y < 64; three ranks on one device give the one-rank image"""
    b = bank(oracle, rpt, world, "DarkCornell")
    y, x = tile_positions(hipmod, 1, 3)
    own = np.zeros((H0, W0), bool)
    own[y, x] = True
    assert own.sum() == 36 * 64
    for name, mask in (("all", np.ones((H0, W0), bool)), ("checkerboard", checkerboard())):
        with fresh(hipmod, world, "DarkCornell", b, partition=(1, 3)) as r:
            r.render_pixels(mask, 5)
            acc = check_counts(r, b, mask * 5, own=own, rendered=int((mask & own).sum()) * 5, what=f"rank 1 of 3, {name}")
            assert not acc[~own].view(np.uint32).any() and r.counts_uniform() == (name == "all")
    m = hipmod.MultiRenderer([0, 0, 0], allow_shared_device=True)
    try:
        m.upload_scene(world("DarkCornell"))
        m.set_config(b.cfg)
        m.reset(b.rng(0))
        m.set_moments(True)
        m.render(3)
        m.render_pixels(checkerboard(), 5)
        counts = 3 + 5 * checkerboard()
        want_acc, _, want_mom = aref.expected_state(b, counts)
        acc, samples = m.read_accum()
        assert samples == 3 and same_words(acc, want_acc) and same_words(m.read_moments(), want_mom) and not m.counts_uniform()
        assert m.stats()["samples"] == int(counts.sum())
        assert m.denoise(params=hipmod.denoise_params(iterations=0)).tobytes() == (want_acc[..., :3] / want_acc[..., 3:4]).tobytes()
        m.reset(b.rng(0))
        assert m.counts_uniform()
        m.render_pixels(np.ones((H0, W0), bool), 4)                 # every pixel of every rank: a uniform call
        acc, samples = m.read_accum()
        assert samples == 4 and same_words(acc, b.accum(4)) and m.counts_uniform()
    finally:
        m.close()


ADAPTIVE = [("VeachMIS", 0.3), ("DarkCornell", 0.2)]


@pytest.mark.parametrize("scene,threshold", ADAPTIVE)
def test_adaptive_run(hipmod, oracle, rpt, world, scene, threshold):
    """min 8, batch 8, max 64: per-pixel counts, accumulator, passes, converged, counts and pixel_samples are the restatement's prediction, exactly.
    (Confirmed from the bank before these parameters were committed: VeachMIS at 0.3 stops 2767 pixels at 8, takes 70 to the cap and uses all eight counts of
    the schedule; DarkCornell at 0.2: 3896 at 8, 116 at the cap.)"""
    b = bank(oracle, rpt, world, scene)
    t = aref.Target(threshold, 0, 8, 8, 64)
    sim = aref.simulate(b, t)
    n = sim["counts_image"]
    print(f"{scene}, threshold {threshold}: predicted {sim['passes']} passes, converged {sim['converged']}, {sim['pixel_samples']} pixel-samples, counts {sim['counts']}, "
          f"pixels per count {dict(zip(*[a.tolist() for a in np.unique(n, return_counts=True)]))}")
    assert (n == 8).any() and (n == 64).any() and len(np.unique(n)) >= 3          # the prediction itself is not trivial
    assert np.array_equal(n, aref.closed_form(b, t))
    with fresh(hipmod, world, scene, b, moments=False) as r:
        res = r.render_adaptive(**t.kwargs())
        print(f"{scene}: device {res}")
        assert r.moments_on() and not r.counts_uniform()
        assert np.array_equal(r.read_moments()[..., 2], n.astype(F))
        check_counts(r, b, n, rendered=sim["pixel_samples"], what=f"{scene}, adaptive")
        assert (res["passes"], res["converged"], res["counts"], res["pixel_samples"]) == (sim["passes"], sim["converged"], sim["counts"], sim["pixel_samples"])
        assert (res["min_pixel_samples"], res["max_pixel_samples"]) == (int(n.min()), int(n.max())) and res["ms"] > 0
    early = aref.Target(threshold, 350, 8, 8, 64)                 # at most 350 above: stops early, converged
    sim2 = aref.simulate(b, early)
    assert sim2["converged"] == 1 and 0 < sim2["passes"] < sim["passes"] and sim2["counts"]["above"] > 0
    with fresh(hipmod, world, scene, b) as r:
        res = r.render_adaptive(**early.kwargs())
        assert (res["passes"], res["converged"], res["counts"], res["pixel_samples"]) == (sim2["passes"], 1, sim2["counts"], sim2["pixel_samples"])
        check_counts(r, b, sim2["counts_image"], rendered=sim2["pixel_samples"], what=f"{scene}, adaptive, at most 350 above")


def test_adaptive_run_over_three_ranks(hipmod, oracle, rpt, world):
    """above and selected are sums over the ranks: the one-rank prediction, whatever the partition"""
    b = bank(oracle, rpt, world, "VeachMIS")
    t = aref.Target(0.3, 0, 8, 8, 64)
    sim = aref.simulate(b, t)
    m = hipmod.MultiRenderer([0, 0, 0], allow_shared_device=True)
    try:
        m.upload_scene(world("VeachMIS"))
        m.set_config(b.cfg)
        m.reset(b.rng(0))
        res = m.render_adaptive(**t.kwargs())
        assert (res["passes"], res["converged"], res["counts"], res["pixel_samples"]) == (sim["passes"], sim["converged"], sim["counts"], sim["pixel_samples"])
        assert (res["min_pixel_samples"], res["max_pixel_samples"]) == (8, 64)
        want_acc, _, want_mom = aref.expected_state(b, sim["counts_image"])
        acc, _ = m.read_accum()
        assert same_words(acc, want_acc) and same_words(m.read_moments(), want_mom) and m.stats()["samples"] == sim["pixel_samples"]
    finally:
        m.close()


def test_refusals_leave_the_context_usable(hipmod, oracle, rpt, world):
    b = bank(oracle, rpt, world, "DarkCornell")
    L = hipmod.lib()
    with fresh(hipmod, world, "DarkCornell", b, moments=False, reset=False) as r:
        for call in (lambda: r.render_pixels(checkerboard(), 1), lambda: r.render_adaptive(0.3)):         # before rpt_reset
            with pytest.raises(hipmod.RptError) as e:
                call()
            assert e.value.code == -1 and "reset" in str(e.value)
        r.reset(b.rng(0))
        assert L.rpt_render_pixels(r._h, None, 1) == -1 and b"null mask" in L.rpt_last_error(r._h)
        res = hipmod.AdaptiveResult()
        assert L.rpt_render_adaptive(r._h, None, C.byref(res)) == -1
        for bad in (dict(threshold=0.3, batch_samples=0), dict(threshold=0.3, min_samples=9, max_samples=8), dict(threshold=-0.1), dict(threshold=float("nan"))):
            with pytest.raises(hipmod.RptError) as e:
                r.render_adaptive(**bad)
            assert e.value.code == -1, bad
        assert r.counts_uniform() and r.read_accum()[1] == 0 and not r.read_accum()[0].any()
        r.render_pixels(checkerboard(), 0)                        # no samples: nothing happens
        assert r.counts_uniform()
        r.render(6)
        check_counts(r, b, np.full((H0, W0), 6), moments=False, rendered=W0 * H0 * 6, what="after the refusals")
