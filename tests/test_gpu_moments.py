"""GPU tests of the per-pixel sample moments (rpt_set_moments, rpt_read_moments, rpt_read_noise, rpt_noise_count, rpt_render_to_noise and their rpt_multi_*
forms; csrc/k_complete.h k_complete_moments, csrc/k_moments.h).

The reference of every case is the numpy restatement of tests/moments_ref.py fed with the CPU oracle's per-sample radiances (one-sample oracle calls chained
through the returned rng): the moments record is compared word for word, the accumulator with the oracle's bit for bit, the ray counts with the oracle's.
Images are 100 x 70 (7 000 pixels: the last chunk of 64 has padding slots) unless stated; DarkCornell lives in LDS, VeachMIS is walked from global memory,
both with nee = 1."""
import numpy as np
import pytest

import moments_ref as ref

pytestmark = pytest.mark.gpu

W0, H0 = 100, 70
F = np.float32
_banks = {}


def bank(oracle, rpt, world, scene, w=W0, h=H0):
    """the per-sample radiances of (scene, nee 1, w x h, blue-noise seeds): computed once for the session, extended on demand, never changed"""
    key = (scene, w, h)
    if key not in _banks:
        _banks[key] = ref.SampleBank(oracle, rpt.default_config(w, h, nee=1), world(scene), rpt.blue_noise_seeds(w, h))
    return _banks[key]


def layout(monkeypatch, q_shift):
    if q_shift is None:
        monkeypatch.delenv("RPT_SLOT_Q_SHIFT", raising=False)
    else:
        monkeypatch.setenv("RPT_SLOT_Q_SHIFT", q_shift)


class fresh:
    """a Renderer of its own (the developer knobs are read by rpt_create), with the scene and configuration of a bank, reset to its seeds"""

    def __init__(self, hipmod, world, scene, b, moments=True, in_flight=None, partition=None):
        self.r = hipmod.Renderer(0) if partition is None else hipmod.Renderer(0, *partition)
        try:
            if in_flight is not None:
                self.r.set_samples_in_flight(in_flight)
            self.r.upload_scene(world(scene))
            self.r.set_config(b.cfg)
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


def check_state(r, b, n, first=0, stats=True):
    """moments == the restatement over the samples first .. n - 1, accumulator == the in-order sum of all n (== the oracle's, checked by the callers that
    render from zero), ray counts == the oracle's"""
    mom = r.read_moments()
    want = b.moments(n, first)
    assert same_words(mom, want), f"{int((mom.view(np.uint32) != want.view(np.uint32)).sum())} moments words differ"
    acc, samples = r.read_accum()
    assert samples == n and same_words(acc, b.accum(n))
    if stats:
        st, want_st = r.stats(), b.ray_counts(n)
        assert {k: st[k] for k in ref.STAT_KEYS} == want_st
    return mom


def check_bank_against_the_oracle(oracle, world, scene, b, n):
    """the bank's in-order sum IS the oracle's n-sample accumulator, and its counts the oracle's"""
    acc, rng, st = oracle.trace_cpu(b.cfg, oracle.scene(world(scene)), b.rng(0), n)
    assert same_words(acc, b.accum(n)) and np.array_equal(rng, b.rng(n))
    assert {k: getattr(st, k) for k in ref.STAT_KEYS} == b.ray_counts(n)


@pytest.mark.parametrize("q_shift", [None, "3"])
@pytest.mark.parametrize("scene", ["DarkCornell", "VeachMIS"])
def test_async_batches_of_changing_length(monkeypatch, hipmod, oracle, rpt, world, scene, q_shift):
    """batches of 5, 8, 3, 16 and 6 samples, asynchronous, one wait: 5 of 8 slots, 3 of 4, 6 of 8 — the completion of each batch adds a prefix of its slots"""
    layout(monkeypatch, q_shift)
    b = bank(oracle, rpt, world, scene)
    batches = (5, 8, 3, 16, 6)
    check_bank_against_the_oracle(oracle, world, scene, b, sum(batches))
    with fresh(hipmod, world, scene, b) as r:
        for n in batches:
            r.render_async(n)
        r.wait()
        mom = check_state(r, b, sum(batches))
        assert np.all(mom[..., 2] == sum(batches)) and mom[..., 3].max() > 0


@pytest.mark.parametrize("q_shift", [None, "3"])
@pytest.mark.parametrize("scene", ["DarkCornell", "VeachMIS"])
def test_slots_that_take_several_samples(monkeypatch, hipmod, oracle, rpt, world, scene, q_shift):
    """4 slots per pixel, 19 samples in one call: the completion runs after every shade stage and restarts the finished slots (slot k takes k, k + 4, ...)"""
    layout(monkeypatch, q_shift)
    b = bank(oracle, rpt, world, scene)
    with fresh(hipmod, world, scene, b, in_flight=4) as r:
        r.render(19)
        check_state(r, b, 19)


@pytest.mark.parametrize("q_shift", [None, "5"])
def test_more_than_32_slots_per_pixel(monkeypatch, hipmod, oracle, rpt, world, q_shift):
    """64 x 48, 64 slots per pixel, one asynchronous batch of 64: with q_shift 5 the tile loop runs two blocks of 32 rows, without it eight row groups"""
    layout(monkeypatch, q_shift)
    b = bank(oracle, rpt, world, "DarkCornell", 64, 48)
    with fresh(hipmod, world, "DarkCornell", b, in_flight=64) as r:
        r.render_async(64)
        r.wait()
        check_state(r, b, 64)


def test_one_sample_calls(hipmod, oracle, rpt, world):
    """six render(1): each uses slot 0 of 2 and passes through the completion kernel; a context with ONE slot per pixel refuses to render while moments are on
    and renders again once they are off"""
    b = bank(oracle, rpt, world, "DarkCornell")
    check_bank_against_the_oracle(oracle, world, "DarkCornell", b, 6)
    with fresh(hipmod, world, "DarkCornell", b) as r:
        for _ in range(6):
            r.render(1)
        check_state(r, b, 6)
    with fresh(hipmod, world, "DarkCornell", b, in_flight=1) as r:
        for call in (r.render, r.render_async):
            with pytest.raises(hipmod.RptError) as e:
                call(1)
            assert e.value.code == -1 and "rpt_set_samples_in_flight" in str(e.value) and "rpt_set_moments" in str(e.value)
        with pytest.raises(hipmod.RptError) as e:
            r.render_to_noise(0.3, max_above=0, batch_samples=8, min_samples=8, max_samples=16)
        assert e.value.code == -1
        assert r.read_accum()[1] == 0 and not r.read_moments().any()
        r.set_moments(False)
        r.render(6)
        acc, n = r.read_accum()
        assert n == 6 and same_words(acc, b.accum(6))


def test_lifecycle(hipmod, oracle, rpt, world):
    b = bank(oracle, rpt, world, "VeachMIS")
    with fresh(hipmod, world, "VeachMIS", b, moments=False) as r:
        assert not r.moments_on()
        for call in (r.read_moments, r.read_noise, lambda: r.noise_count(0.1)):
            with pytest.raises(hipmod.RptError) as e:
                call()
            assert e.value.code == -1 and "moments are off" in str(e.value)
        r.render(8)
        r.set_moments(True)                               # turned on after 8 samples: the record holds exactly the samples 8 .. 23 after 16 more
        assert r.moments_on() and not r.read_moments().any()
        r.render_async(16)
        mom = check_state(r, b, 24, first=8)
        assert np.all(mom[..., 2] == 16)
        r.reset(b.rng(0))                                 # rpt_reset zeroes them
        assert not r.read_moments().any() and r.moments_on()
        r.reset(b.rng(8), b.accum(8), 8)                  # resumed: accum.w continues from 8, m.z starts at 0
        r.render(8)
        mom = check_state(r, b, 16, first=8, stats=False)
        assert np.all(mom[..., 2] == 8) and np.all(r.read_accum()[0][..., 3] == 16)
        r.set_config(rpt.default_config(64, 48, nee=1))   # a resize zeroes them (and sizes them anew)
        r.reset(rpt.blue_noise_seeds(64, 48))
        assert r.read_moments().shape == (48, 64, 4) and not r.read_moments().any()
        r.render(3)
        assert np.all(r.read_moments()[..., 2] == 3)
    # on, off and on again mid-run: accumulator, rng and ray counts of a context that never did
    with fresh(hipmod, world, "VeachMIS", b, moments=False) as r:
        r.render_async(5)
        r.set_moments(True)
        r.render_async(8)
        r.set_moments(False)
        r.render(3)
        r.set_moments(True)
        r.render_async(8)
        mom = r.read_moments()
        assert same_words(mom, b.moments(24, first=16))
        acc, n = r.read_accum()
        st = r.stats()
        assert n == 24 and same_words(acc, b.accum(24)) and np.array_equal(r.read_rng().reshape(-1), np.asarray(b.rng(24)).reshape(-1))
        assert {k: st[k] for k in ref.STAT_KEYS} == b.ray_counts(24)
    with fresh(hipmod, world, "VeachMIS", b, moments=False) as r:
        for n in (5, 8, 3, 8):
            r.render_async(n)
        acc, n = r.read_accum()
        assert n == 24 and same_words(acc, b.accum(24)) and np.array_equal(r.read_rng().reshape(-1), np.asarray(b.rng(24)).reshape(-1))


def test_partition_and_multi_gpu(hipmod, oracle, rpt, world, tiles):
    """200 x 130: six tiles of 64 x 64, rank 1 of 3 owns two of them"""
    w, h = 200, 130
    b = bank(oracle, rpt, world, "DarkCornell", w, h)
    whole = b.moments(8)
    xy = hipmod.tile_order(w, h, 1, 3)
    own = np.zeros((h, w), bool)
    own[xy >> 16, xy & 0xFFFF] = True
    with fresh(hipmod, world, "DarkCornell", b, partition=(1, 3)) as r:
        r.render_async(8)
        mom = r.read_moments()
        assert same_words(mom[own], whole[own]) and not mom[~own].any()
        noise = r.read_noise()
        assert ref.same_bits(noise[own], ref.noise_rel(whole)[own]) and not noise[~own].any()
        counts = r.noise_count(0.3)
        assert counts["pixels"] == r.rank_pixels(1) == own.sum() and counts == ref.noise_counts(whole[own], 0.3)
    with fresh(hipmod, world, "DarkCornell", b) as r:
        r.render_async(8)
        one_mom, one_counts = r.read_moments(), r.noise_count(0.3)
        assert same_words(one_mom, whole) and one_counts == ref.noise_counts(whole, 0.3)
    m = hipmod.MultiRenderer([0, 0], allow_shared_device=True)
    try:
        m.upload_scene(world("DarkCornell"))
        m.set_config(b.cfg)
        m.reset(b.rng(0))
        m.set_moments(True)
        assert m.moments_on()
        m.render(8)
        assert same_words(m.read_moments(), one_mom) and m.noise_count(0.3) == one_counts
        assert ref.same_bits(m.read_noise(), ref.noise_rel(whole))
        acc, n = m.read_accum()
        assert n == 8 and same_words(acc, b.accum(8))
        res = m.render_to_noise(0.3, max_above=w * h, batch_samples=8, min_samples=8, max_samples=16)     # every count passes: one batch
        assert res["samples_rendered"] == 8 and res["converged"] == 1 and res["counts"] == ref.noise_counts(b.moments(16), 0.3)
        acc, n = m.read_accum()
        assert n == 16 and same_words(acc, b.accum(16))
    finally:
        m.close()


def test_partition_read_outs(hipmod, oracle, rpt, world):
    """200 x 130, rank 1 of 3, 8 samples — the rank owns two whole 64 x 64 tiles, an 8 x 64 one of the right edge and a 64 x 2 one of the bottom edge: every
    row-major read-out of the partitioned context holds the oracle's values on the rank's own pixels and zeros elsewhere, and after an asynchronous batch
    resolve and read_rng return without an explicit wait what they return after one"""
    w, h = 200, 130
    b = bank(oracle, rpt, world, "DarkCornell", w, h)
    check_bank_against_the_oracle(oracle, world, "DarkCornell", b, 8)
    xy = hipmod.tile_order(w, h, 1, 3)
    own = np.zeros((h, w), bool)
    own[xy >> 16, xy & 0xFFFF] = True
    assert own.sum() == 2 * 64 * 64 + 8 * 64 + 64 * 2 and own[:64, 64:128].all() and own[64:128, :64].all() and own[64:128, 192:].all() and own[128:, 128:192].all()
    want_acc, want_rng = b.accum(8), np.asarray(b.rng(8)).reshape(h, w)
    want_rgb = {op: oracle.resolve(want_acc, 8.0, op) for op in (0, 4)}

    def read_rng(r):
        rng = r.read_rng().reshape(h, w)
        assert np.array_equal(rng[own], want_rng[own]) and not rng[~own].view(np.uint32).any()
        return rng

    def resolve(r, op=0):
        rgb = r.resolve(op)
        assert same_words(rgb[own], want_rgb[op][own]) and not rgb[~own].view(np.uint32).any(), op
        return rgb

    with fresh(hipmod, world, "DarkCornell", b, moments=False, partition=(1, 3)) as r:
        r.render_async(8)
        r.wait()
        acc, n = r.read_accum()
        assert n == 8 and same_words(acc[own], want_acc[own]) and not acc[~own].view(np.uint32).any()
        waited = {read_rng: read_rng(r), resolve: resolve(r)}
        resolve(r, 4)                                     # ACES (Hill): a curved operator
    for first, second in ((resolve, read_rng), (read_rng, resolve)):
        with fresh(hipmod, world, "DarkCornell", b, moments=False, partition=(1, 3)) as r:
            r.render_async(8)                             # no wait: the read-out has to
            for read in (first, second):
                assert read(r).tobytes() == waited[read].tobytes()


@pytest.mark.parametrize("scene", ["DarkCornell", "VeachMIS"])
def test_noise(hipmod, oracle, rpt, world, scene):
    b = bank(oracle, rpt, world, scene)
    with fresh(hipmod, world, scene, b) as r:
        r.render_async(8)
        r.render_async(8)
        mom = check_state(r, b, 16)
        noise, want = r.read_noise(), ref.noise_rel(b.moments(16))
        assert ref.same_bits(noise, hipmod.noise_host(mom)[0]) and ref.same_bits(noise, want)
        assert np.isfinite(noise).all() and (noise > 0).sum() > 1000
        for t in (0.0, 0.1, 0.3, float("inf")):
            assert r.noise_count(t) == ref.noise_counts(mom, t), t
        for t in (-1.0, float("nan")):
            with pytest.raises(hipmod.RptError) as e:
                r.noise_count(t)
            assert e.value.code == -1
    with fresh(hipmod, world, scene, b) as r:             # one sample: nothing is measured, every rel is +inf
        r.render(1)
        assert np.all(np.isposinf(r.read_noise())) and r.noise_count(0.3) == {"pixels": W0 * H0, "measured": 0, "above": 0}


def predicted_stop(b, threshold, max_above, batch, min_samples, max_samples):
    """what rpt_render_to_noise must do, from the restatement alone: (samples rendered, converged, the last counts)"""
    n, counts = 0, None
    while n < max_samples:
        n += min(batch, max_samples - n)
        if n < min_samples:
            continue
        counts = ref.noise_counts(b.moments(n), threshold)
        if counts["measured"] == counts["pixels"] and counts["above"] <= max_above:
            return n, 1, counts
    return n, 0, counts


def test_render_to_a_noise_target(hipmod, oracle, rpt, world):
    b = bank(oracle, rpt, world, "VeachMIS")
    target = dict(threshold=0.3, max_above=350, batch_samples=8, min_samples=8, max_samples=128)
    n, converged, counts = predicted_stop(b, 0.3, 350, 8, 8, 128)
    print(f"VeachMIS 100 x 70, threshold 0.3, at most 350 above: the restatement stops at {n} samples, counts {counts}")
    assert converged == 1 and 8 < n < 128
    check_bank_against_the_oracle(oracle, world, "VeachMIS", b, n)
    with fresh(hipmod, world, "VeachMIS", b, moments=False) as r:
        res = r.render_to_noise(**target)
        assert res["samples_rendered"] == n and res["converged"] == 1 and res["counts"] == counts and res["ms"] > 0
        assert r.moments_on()                             # turned on, left on
        check_state(r, b, n)
    with fresh(hipmod, world, "VeachMIS", b) as r:        # a target out of reach runs to its cap
        assert predicted_stop(b, 0.05, 350, 8, 8, 64)[:2] == (64, 0)
        check_bank_against_the_oracle(oracle, world, "VeachMIS", b, 64)
        res = r.render_to_noise(0.05, max_above=350, batch_samples=8, min_samples=8, max_samples=64)
        assert res["samples_rendered"] == 64 and res["converged"] == 0 and res["counts"] == ref.noise_counts(b.moments(64), 0.05)
        check_state(r, b, 64)
    with fresh(hipmod, world, "VeachMIS", b) as r:        # batches of 24 up to 40: the second one is clipped to 16
        before = r.stats()["kernel_launches"]["generate"]
        res = r.render_to_noise(0.05, max_above=350, batch_samples=24, min_samples=8, max_samples=40)
        assert res["samples_rendered"] == 40 and res["converged"] == 0 and r.stats()["kernel_launches"]["generate"] - before == 2
        check_state(r, b, 40)
        # invalid targets: refused, nothing rendered, the context stays usable
        for bad in (dict(threshold=0.3, batch_samples=0), dict(threshold=0.3, min_samples=9, max_samples=8), dict(threshold=-0.1), dict(threshold=float("nan"))):
            with pytest.raises(hipmod.RptError) as e:
                r.render_to_noise(**bad)
            assert e.value.code == -1, bad
        assert r.read_accum()[1] == 40
        res = r.render_to_noise(float("inf"), max_above=0, batch_samples=8, min_samples=0, max_samples=64)   # nothing is above +inf: one batch
        assert res["samples_rendered"] == 8 and res["converged"] == 1 and res["counts"]["above"] == 0
        check_state(r, b, 48)
