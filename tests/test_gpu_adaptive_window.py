"""GPU tests of adaptive sampling by a pixel's neighbourhood (rpt_render_adaptive_window, rpt_adaptive_mask and their rpt_multi_* forms; csrc/k_adaptive.h
k_ad_window, rpt_adaptive.hip).

The contract is the one of tests/test_gpu_adaptive.py, whose banks and helpers are used here: a pixel that has received N samples by any route holds, bit for bit,
what the CPU oracle holds after N samples.  What is new is WHICH pixels a pass selects: the mask is held to tests/adaptive_window_ref.py select (shifted boolean
images per tile, nothing of the kernel's row words), and a whole call to its pass-by-pass simulation — per-pixel counts, accumulator, rng and moments word for
word, and every field of the result but ms.  Images are 100 x 70 with nee 1 (four tiles: 64 x 64, 36 x 64, 64 x 6, 36 x 6 — one full tile, three partial);
the mask is also checked at 130 x 67 and 65 x 65 (tiles one pixel wide and high)."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as aref
import adaptive_window_ref as awr
import moments_ref as ref
from test_gpu_adaptive import ADAPTIVE, H0, W0, bank, check_counts, fresh, same_words

pytestmark = pytest.mark.gpu

F = np.float32
_small = {}


def target(threshold, max_above=0, cap=64):
    return aref.Target(threshold, max_above, 8, 8, cap)


def result_fields(res):
    return {k: v for k, v in res.items() if k != "ms"}


def predicted_fields(sim):
    n = sim["counts_image"]
    return {"passes": sim["passes"], "converged": sim["converged"], "min_pixel_samples": int(n.min()), "max_pixel_samples": int(n.max()),
            "pixel_samples": sim["pixel_samples"], "counts": sim["counts"]}


def state(r):
    return r.read_accum()[0].tobytes(), r.read_accum()[1], r.read_rng().tobytes(), r.read_moments().tobytes(), r.stats()["samples"], r.counts_uniform()


def nontrivial(sim, what):
    n = sim["counts_image"]
    print(f"{what}: predicted {sim['passes']} passes, converged {sim['converged']}, {sim['pixel_samples']} pixel-samples, counts {sim['counts']}, "
          f"pixels per count {dict(zip(*[a.tolist() for a in np.unique(n, return_counts=True)]))}, selected per pass {sim['selected_per_pass']}")
    assert (n == 8).any() and (n == 64).any() and len(np.unique(n)) >= 3, what


@pytest.mark.parametrize("scene,threshold", ADAPTIVE)
def test_mask_after_eight_samples(hipmod, oracle, rpt, world, scene, threshold):
    """adaptive_mask == the restatement on bank.moments(8), counts included, for radius 0, 1, 3 and 8; the call leaves accumulator, rng, moments and stats alone;
    and render_pixels(that mask, 8) is one pass of the simulation"""
    b = bank(oracle, rpt, world, scene)
    t = target(threshold)
    m8 = b.moments(8)
    with fresh(hipmod, world, scene, b) as r:
        r.render(8)
        before = state(r)
        sizes = []
        for radius in (0, 1, 3, 8):
            mask, counts = r.adaptive_mask(radius, **t.kwargs())
            want = awr.select(m8, threshold, 8, 64, radius)
            sizes.append(int(want.sum()))
            assert mask.dtype == np.uint8 and mask.max() <= 1 and np.array_equal(mask.astype(bool), want), (scene, radius, int((mask.astype(bool) != want).sum()))
            assert counts == ref.noise_counts(m8, threshold), (scene, radius)
            assert state(r) == before, (scene, radius)
        print(f"{scene}: selected after 8 samples for radius 0, 1, 3, 8: {sizes}")
        assert 0 < sizes[0] < sizes[1] < sizes[2] < sizes[3] == W0 * H0
        mask, _ = r.adaptive_mask(1, **t.kwargs())
        r.render_pixels(mask, 8)
        check_counts(r, b, 8 + 8 * mask.astype(np.int64), rendered=W0 * H0 * 8 + int(mask.sum()) * 8, what=f"{scene}, one pass by hand")
        second, counts = r.adaptive_mask(1, **t.kwargs())                 # and the next mask is the simulation's second selection
        m = aref.moments_at(b, 8 + 8 * mask.astype(np.int64))
        assert np.array_equal(second.astype(bool), awr.select(m, threshold, 8, 64, 1)) and counts == ref.noise_counts(m, threshold)


@pytest.mark.parametrize("w,h", [(130, 67), (65, 65)])
def test_mask_at_other_tilings(hipmod, oracle, rpt, world, w, h):
    """3 x 2 tiles with a last column 2 pixels wide and a last row 3 tall; 2 x 2 tiles of 64 x 64, 1 x 64, 64 x 1 and 1 x 1 pixels"""
    if (w, h) not in _small:
        _small[(w, h)] = ref.SampleBank(oracle, rpt.default_config(w, h, nee=1), world("DarkCornell"), rpt.blue_noise_seeds(w, h))
    b = _small[(w, h)]
    m8 = b.moments(8)
    t = target(0.2)
    with fresh(hipmod, world, "DarkCornell", b) as r:
        r.render(8)
        assert same_words(r.read_moments(), m8)
        for radius in (0, 1, 3, 8):
            mask, counts = r.adaptive_mask(radius, **t.kwargs())
            want = awr.select(m8, 0.2, 8, 64, radius)
            assert np.array_equal(mask.astype(bool), want) and counts == ref.noise_counts(m8, 0.2), (w, h, radius, int((mask.astype(bool) != want).sum()))
            assert 0 < want.sum()
        assert not awr.select(m8, 0.2, 8, 64, 3).all()


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("scene,threshold", ADAPTIVE)
def test_full_run(hipmod, oracle, rpt, world, scene, threshold, radius):
    """min 8, batch 8, max 64: per-pixel counts, accumulator, rng, moments and every field of the result are the simulation's, exactly"""
    b = bank(oracle, rpt, world, scene)
    t = target(threshold)
    sim = awr.simulate(b, t, radius)
    nontrivial(sim, f"{scene}, radius {radius}")
    n = sim["counts_image"]
    assert not np.array_equal(n, aref.closed_form(b, t))                  # pixels below the threshold were selected again
    with fresh(hipmod, world, scene, b, moments=False) as r:
        res = r.render_adaptive_window(radius, **t.kwargs())
        print(f"{scene}, radius {radius}: device {res}")
        assert r.moments_on() and not r.counts_uniform()
        assert np.array_equal(r.read_moments()[..., 2], n.astype(F))
        check_counts(r, b, n, rendered=sim["pixel_samples"], what=f"{scene}, radius {radius}")
        assert result_fields(res) == predicted_fields(sim) and res["ms"] > 0


def test_a_run_that_stops_early(hipmod, oracle, rpt, world):
    """at most 350 above: converged before the cap, as the simulation says"""
    b = bank(oracle, rpt, world, "VeachMIS")
    full, t = awr.simulate(b, target(0.3), 1), target(0.3, 350)
    sim = awr.simulate(b, t, 1)
    assert sim["converged"] == 1 and 0 < sim["passes"] < full["passes"] and sim["counts"]["above"] > 0
    with fresh(hipmod, world, "VeachMIS", b) as r:
        res = r.render_adaptive_window(1, **t.kwargs())
        assert result_fields(res) == predicted_fields(sim)
        check_counts(r, b, sim["counts_image"], rendered=sim["pixel_samples"], what="VeachMIS, radius 1, at most 350 above")


@pytest.mark.parametrize("scene,threshold", ADAPTIVE)
def test_radius_8_begins_with_uniform_passes(hipmod, oracle, rpt, world, scene, threshold):
    """the first mask selects every pixel: that pass runs as the uniform call it amounts to (cap 16: it is the only one, and the context is what render(16)
    leaves, counts uniform); with cap 64 the call goes on to partial passes and ends as the simulation says"""
    b = bank(oracle, rpt, world, scene)
    sim = awr.simulate(b, target(threshold), 8)
    print(f"{scene}, radius 8: predicted {sim['passes']} passes, selected per pass {sim['selected_per_pass']}")
    assert sim["first_mask"].all() and sim["selected_per_pass"][-1] < W0 * H0 and len(np.unique(sim["counts_image"])) >= 2
    short = awr.simulate(b, target(threshold, cap=16), 8)
    assert short["passes"] == 1 and (short["counts_image"] == 16).all()
    with fresh(hipmod, world, scene, b) as r:
        res = r.render_adaptive_window(8, **target(threshold, cap=16).kwargs())
        assert result_fields(res) == predicted_fields(short)
        acc, samples = r.read_accum()
        assert r.counts_uniform() and samples == 16 and same_words(acc, b.accum(16)) and same_words(r.read_moments(), b.moments(16))
        assert r.stats()["samples"] == W0 * H0 * 16
    with fresh(hipmod, world, scene, b) as r:
        res = r.render_adaptive_window(8, **target(threshold).kwargs())
        assert result_fields(res) == predicted_fields(sim) and not r.counts_uniform()
        whole = sum(s == W0 * H0 for s in sim["selected_per_pass"])
        assert r.read_accum()[1] == 8 + 8 * whole                            # the uniform count grew by the passes that selected every pixel, and by no other
        check_counts(r, b, sim["counts_image"], rendered=sim["pixel_samples"], what=f"{scene}, radius 8")


@pytest.mark.parametrize("scene,threshold", ADAPTIVE)
def test_radius_0_is_render_adaptive(hipmod, oracle, rpt, world, scene, threshold):
    """every word of the state and every field of the result but ms"""
    b = bank(oracle, rpt, world, scene)
    t = target(threshold)
    with fresh(hipmod, world, scene, b) as r, fresh(hipmod, world, scene, b) as q:
        res, want = r.render_adaptive_window(0, **t.kwargs()), q.render_adaptive(**t.kwargs())
        assert result_fields(res) == result_fields(want) and res["passes"] > 0
        assert state(r) == state(q)
        assert r.resolve(0).tobytes() == q.resolve(0).tobytes()


def test_ranks_select_their_share_of_the_one_rank_mask(hipmod, oracle, rpt, world):
    b = bank(oracle, rpt, world, "DarkCornell")
    t = target(0.2)
    m8 = b.moments(8)
    for rank, size in ((0, 2), (1, 2), (2, 3)):
        own = awr.owned(W0, H0, rank, size)
        with fresh(hipmod, world, "DarkCornell", b, partition=(rank, size)) as r:
            r.render(8)
            for radius in (1, 3):
                mask, counts = r.adaptive_mask(radius, **t.kwargs())
                assert np.array_equal(mask.astype(bool), awr.select(m8, 0.2, 8, 64, radius) & own), (rank, size, radius)
                assert counts == ref.noise_counts(m8[own], 0.2)


def test_three_ranks_give_the_one_rank_image(hipmod, oracle, rpt, world):
    b = bank(oracle, rpt, world, "VeachMIS")
    t = target(0.3)
    sim = awr.simulate(b, t, 1)
    m = hipmod.MultiRenderer([0, 0, 0], allow_shared_device=True)
    try:
        m.upload_scene(world("VeachMIS"))
        m.set_config(b.cfg)
        m.reset(b.rng(0))
        m.set_moments(True)
        m.render(8)
        mask, counts = m.adaptive_mask(1, **t.kwargs())
        assert np.array_equal(mask.astype(bool), sim["first_mask"]) and counts == ref.noise_counts(b.moments(8), 0.3)
        m.reset(b.rng(0))                                                  # (zeroes the moments record and the statistics)
        res = m.render_adaptive_window(1, **t.kwargs())
        assert result_fields(res) == predicted_fields(sim)
        want_acc, _, want_mom = aref.expected_state(b, sim["counts_image"])
        acc, _ = m.read_accum()
        assert same_words(acc, want_acc) and same_words(m.read_moments(), want_mom) and m.stats()["samples"] == sim["pixel_samples"]
    finally:
        m.close()


def test_both_slot_layouts(monkeypatch, hipmod, oracle, rpt, world):
    """RPT_SLOT_Q_SHIFT=3, and four samples of a pixel in flight (the polled path).  With ONE sample in flight a context with moments on refuses to render
    (tests/test_gpu_moments.py), so this call is refused there too, and the context stays usable."""
    b = bank(oracle, rpt, world, "DarkCornell")
    t = target(0.2)
    sim = awr.simulate(b, t, 1)
    with fresh(hipmod, world, "DarkCornell", b, in_flight=4) as r:
        assert result_fields(r.render_adaptive_window(1, **t.kwargs())) == predicted_fields(sim)
        check_counts(r, b, sim["counts_image"], rendered=sim["pixel_samples"], what="four in flight")
    with fresh(hipmod, world, "DarkCornell", b, moments=False, in_flight=1) as r:
        with pytest.raises(hipmod.RptError) as e:
            r.render_adaptive_window(1, **t.kwargs())
        assert e.value.code == -1
        r.set_moments(False)
        r.reset(b.rng(0))
        r.render(3)
        check_counts(r, b, np.full((H0, W0), 3), moments=False, rendered=None, what="one in flight, after the refusal")
    monkeypatch.setenv("RPT_SLOT_Q_SHIFT", "3")
    with fresh(hipmod, world, "DarkCornell", b) as r:
        assert result_fields(r.render_adaptive_window(1, **t.kwargs())) == predicted_fields(sim)
        check_counts(r, b, sim["counts_image"], rendered=sim["pixel_samples"], what="q_shift 3")


def test_refusals_leave_the_context_usable(hipmod, oracle, rpt, world):
    b = bank(oracle, rpt, world, "DarkCornell")
    L = hipmod.lib()
    t = hipmod.NoiseTarget(0.2, 8, 64, 8, 0)
    res, mask = hipmod.AdaptiveResult(), np.zeros((H0, W0), np.uint8)
    bare = hipmod.Renderer(0)                                              # before scene and config
    try:
        assert L.rpt_render_adaptive_window(bare._h, C.byref(t), 1, C.byref(res)) == -1
        assert L.rpt_adaptive_mask(bare._h, C.byref(t), 1, hipmod.ptr(mask), None) == -1
    finally:
        bare.close()
    with fresh(hipmod, world, "DarkCornell", b, moments=False, reset=False) as r:
        with pytest.raises(hipmod.RptError) as e:                          # before rpt_reset
            r.render_adaptive_window(1, 0.2)
        assert e.value.code == -1 and "reset" in str(e.value)
        assert L.rpt_adaptive_mask(r._h, C.byref(t), 1, hipmod.ptr(mask), None) == -1 and b"reset" in L.rpt_last_error(r._h)
        r.reset(b.rng(0))
        with pytest.raises(hipmod.RptError) as e:                          # moments are off
            r.adaptive_mask(1, 0.2)
        assert e.value.code == -1 and "moments" in str(e.value)
        r.set_moments(True)
        for radius in (9, 1 << 31):
            with pytest.raises(hipmod.RptError) as e:
                r.render_adaptive_window(radius, 0.2)
            assert e.value.code == -1 and "radius" in str(e.value)
            with pytest.raises(hipmod.RptError) as e:
                r.adaptive_mask(radius, 0.2)
            assert e.value.code == -1 and "radius" in str(e.value)
        assert L.rpt_render_adaptive_window(r._h, None, 1, C.byref(res)) == -1 and L.rpt_render_adaptive_window(r._h, C.byref(t), 1, None) == -1
        assert L.rpt_render_adaptive_window(None, C.byref(t), 1, C.byref(res)) == -1 and L.rpt_adaptive_mask(None, C.byref(t), 1, hipmod.ptr(mask), None) == -1
        assert L.rpt_adaptive_mask(r._h, None, 1, hipmod.ptr(mask), None) == -1
        assert L.rpt_adaptive_mask(r._h, C.byref(t), 1, None, None) == -1 and b"mask_out" in L.rpt_last_error(r._h)
        for bad in (dict(threshold=0.3, batch_samples=0), dict(threshold=0.3, min_samples=9, max_samples=8), dict(threshold=-0.1), dict(threshold=float("nan"))):
            with pytest.raises(hipmod.RptError) as e:
                r.render_adaptive_window(1, **bad)
            assert e.value.code == -1, bad
            with pytest.raises(hipmod.RptError) as e:
                r.adaptive_mask(1, **bad)
            assert e.value.code == -1, bad
        assert not mask.any() and r.counts_uniform() and r.read_accum()[1] == 0 and not r.read_accum()[0].any()
        full, counts = r.adaptive_mask(1, 0.2, max_samples=64)             # nothing rendered yet: every record is unmeasured, every pixel is selected
        assert full.all() and counts == {"pixels": W0 * H0, "measured": 0, "above": 0}
        r.render(6)
        check_counts(r, b, np.full((H0, W0), 6), rendered=W0 * H0 * 6, what="after the refusals")
    m = hipmod.MultiRenderer([0, 0], allow_shared_device=True)
    try:
        m.upload_scene(world("DarkCornell"))
        m.set_config(b.cfg)
        m.reset(b.rng(0))
        with pytest.raises(hipmod.RptError) as e:
            m.adaptive_mask(1, 0.2)
        assert e.value.code == -1 and "moments" in str(e.value)
        with pytest.raises(hipmod.RptError) as e:
            m.render_adaptive_window(9, 0.2)
        assert e.value.code == -1 and "radius" in str(e.value)
        m.render(2)
        acc, samples = m.read_accum()
        assert samples == 2 and same_words(acc, b.accum(2))
    finally:
        m.close()
