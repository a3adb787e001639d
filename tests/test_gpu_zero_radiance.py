"""GPU tests of the implicit zero radiance of a batch of known length without NEE with several slots per pixel (csrc/k_common.h HIT_DONE_ZERO,
DevQueues::implicit_zero): a live path keeps no radiance record, a path that ends with nothing added ends as HIT_DONE_ZERO with no record, one that ends
with something added (the front of an emitter, the sky) writes 0 + its term and HIT_DONE, and k_complete loads the record of the second kind only.

Every image is compared with the CPU oracle bit for bit and every ray count with the oracle's; the moments record with the restatement of
tests/moments_ref.py.  Both slot layouts (RPT_SLOT_Q_SHIFT unset: a wave is 64 pixels at one sample index, k_complete adds straight from registers; 3: eight
samples of eight pixels, k_complete goes through its LDS tile).  The oracle's images are computed once per case and shared by the layouts.
"""
import numpy as np
import pytest

import moments_ref as ref
import test_gpu_batch_seam as seam

pytestmark = pytest.mark.gpu

W0, H0 = 100, 70            # 7 000 pixels: not a multiple of 64, the last chunk of 64 pixels has padding slots
BATCHES = (32, 5, 64)       # 32 of 32 slots; 5 of 8 (three slots of every pixel stay idle); 64 of 64, into slots the first batch left behind
_cache = {}


def layout(monkeypatch, q_shift):
    monkeypatch.delenv("RPT_LAST_ORDER", raising=False)
    monkeypatch.delenv("RPT_SHADE_COMPACT", raising=False)
    if q_shift is None:
        monkeypatch.delenv("RPT_SLOT_Q_SHIFT", raising=False)
    else:
        monkeypatch.setenv("RPT_SLOT_Q_SHIFT", q_shift)


def the_scene(rpt, world, name):
    """(world, view): the shipped DarkCornell (closed: nearly every path ends with nothing), the lamp box as built and flipped (paths end on the emitter's
    front and on its back), the open tray (sky endings carry radiance)"""
    if name not in _cache:
        _cache[name] = {"DarkCornell": lambda: (world("DarkCornell"), {}), "lamp_box": lambda: (seam.lamp_box_scene(rpt, False), seam.LAMP_VIEW),
                        "lamp_box_flipped": lambda: (seam.lamp_box_scene(rpt, True), seam.LAMP_VIEW), "tray": lambda: (seam.tray_scene(rpt), seam.TRAY_VIEW)}[name]()
    return _cache[name]


def oracle_image(oracle, key, cfg, w, seeds, spp):
    """the oracle's accumulator and statistics of a case: computed once, shared by the layouts, never changed"""
    if key not in _cache:
        acc, rng, st = oracle.trace_cpu(cfg, oracle.scene(w), seeds, spp)
        acc.setflags(write=False)
        _cache[key] = (acc, rng, st)
    return _cache[key]


def same_as(acc, st, want):
    acc_c, _, st_c = want
    assert st["extension_rays"] == st_c.extension_rays and st["sky_evals"] == st_c.sky_evals and st["shadow_rays"] == st_c.shadow_rays
    assert ref.same_bits(acc, acc_c), f"{int((acc.view(np.uint32) != acc_c.view(np.uint32)).sum())} accumulator words differ"


@pytest.mark.parametrize("q_shift", [None, "3"])
@pytest.mark.parametrize("scene", ["DarkCornell", "lamp_box", "lamp_box_flipped", "tray"])
def test_batches_of_32_5_and_64_samples_on_one_context(monkeypatch, hipmod, oracle, rpt, world, scene, q_shift):
    """100 x 70, asynchronous batches of 32, 5 and 64 samples on one context: a HIT_DONE word or a radiance record an earlier batch left in a slot would be
    added by a later one.  max_bounces 4: the three LDS scenes built here end their paths in the LAST walk, all of them pass through three shade launches."""
    layout(monkeypatch, q_shift)
    w, view = the_scene(rpt, world, scene)
    cfg = rpt.default_config(W0, H0, nee=0, min_bounces=3, max_bounces=4, **view)
    seeds = rpt.blue_noise_seeds(W0, H0)
    want = oracle_image(oracle, ("batches", scene), cfg, w, seeds, sum(BATCHES))
    acc, st, st0, last_walk = seam._render(hipmod, w, cfg, seeds, BATCHES)
    assert last_walk
    assert st["kernel_launches"]["shade"] - st0["kernel_launches"]["shade"] == 3 and st["kernel_launches"]["complete"] - st0["kernel_launches"]["complete"] == 1
    same_as(acc, st, want)
    if scene == "tray":
        assert want[2].sky_evals > 0.3 * W0 * H0 * sum(BATCHES)          # the scene is fit for the purpose: sky endings in bulk


MIXED_W = MIXED_H = 64      # one 64 x 64 tile: 64 chunks of 64 pixels
MIXED_SPP = 32
MIXED_VIEW = dict(cam_position=(0.0, 1.0, -1.9, 0.0), cam_rotation=(-0.5, 0.0, 0.0, 0.0))     # looking up at the lamp's front: it fills some chunks and cuts through others


def mixed_chunk_census(hipmod, bank):
    """from the oracle alone: per chunk of 64 pixels (consecutive entries of the tile order) and sample index — a ROW of k_complete at q_shift 0 — how many of
    its 64 samples ended with radiance (in the closed lamp box: on the emitter's front; anything else ends with zeros)"""
    xy = hipmod.tile_order(MIXED_W, MIXED_H, 0, 1)
    x, y = (xy & 0xFFFF).astype(np.int64), (xy >> 16).astype(np.int64)
    bank.need(MIXED_SPP)
    lit = np.stack([np.any(bank.radiance[k][y, x] != 0, axis=-1) for k in range(MIXED_SPP)])          # [sample][pixel in tile order]
    return lit.reshape(MIXED_SPP, -1, 64).sum(axis=2)                                                 # [sample][chunk]


@pytest.mark.parametrize("q_shift", [None, "3"])
def test_rows_that_mix_both_finished_words(monkeypatch, hipmod, oracle, rpt, q_shift):
    """The lamp box at 64 x 64 seen from below the lamp, 32 samples in one batch: the emitter's front fills some chunks of 64 pixels (rows of 64 records) and covers
    part of others, whose rows hold samples that ended on it (HIT_DONE, a record) beside samples that ended with nothing (HIT_DONE_ZERO, none); in the chunks
    away from it a few paths per row find the lamp after a bounce, and some rows hold not a single record: they issue no load."""
    layout(monkeypatch, q_shift)
    w = seam.lamp_box_scene(rpt, False)
    cfg = rpt.default_config(MIXED_W, MIXED_H, nee=0, min_bounces=3, max_bounces=4, **MIXED_VIEW)
    seeds = rpt.blue_noise_seeds(MIXED_W, MIXED_H)
    if "mixed" not in _cache:
        _cache["mixed"] = ref.SampleBank(oracle, cfg, w, seeds)
    bank = _cache["mixed"]
    per_row = mixed_chunk_census(hipmod, bank)
    mixed, none, full = int(((per_row > 0) & (per_row < 64)).sum()), int((per_row == 0).sum()), int((per_row == 64).sum())
    print(f"lamp box {MIXED_W} x {MIXED_H} x {MIXED_SPP}: of {per_row.size} rows {mixed} mix both words, {none} hold no record, {full} hold 64")
    assert mixed >= 1000 and none >= 8 and full >= 8                      # the view is fit for the purpose
    assert int(((per_row > 0).any(axis=0) & (per_row == 0).any(axis=0)).sum()) >= 4      # chunks that have rows with records and rows without
    acc, st, _, last_walk = seam._render(hipmod, w, cfg, seeds, (MIXED_SPP,))
    assert last_walk
    assert ref.same_bits(acc, bank.accum(MIXED_SPP))
    assert {k: st[k] for k in ref.STAT_KEYS} == bank.ray_counts(MIXED_SPP)


@pytest.mark.parametrize("q_shift", [None, "3"])
@pytest.mark.parametrize("mode", ["nee 1", "nee 2", "slots take several samples", "one slot per pixel"])
def test_modes_that_keep_their_radiance_records(monkeypatch, hipmod, oracle, rpt, world, mode, q_shift):
    """What the change must not touch, DarkCornell at 100 x 70: both kinds of NEE in batches of known length; without NEE a call whose slots take several
    samples (19 samples on 4 slots: polled, completed after every shade stage, finished slots restarted) and a context with one slot per pixel (every stage
    accumulates in place)."""
    layout(monkeypatch, q_shift)
    w = world("DarkCornell")
    nee = {"nee 1": 1, "nee 2": 2}.get(mode, 0)
    in_flight, calls = {"slots take several samples": (4, (19,)), "one slot per pixel": (1, (3, 2))}.get(mode, (0, (8, 8)))
    cfg = rpt.default_config(W0, H0, nee=nee)
    seeds = rpt.blue_noise_seeds(W0, H0)
    want = oracle_image(oracle, ("modes", mode), cfg, w, seeds, sum(calls))
    r = hipmod.Renderer(0)
    try:
        r.set_samples_in_flight(in_flight)
        r.upload_scene(w); r.set_config(cfg); r.reset(seeds)
        for n in calls:
            r.render_async(n)
        r.wait()
        acc, n = r.read_accum()
        assert n == sum(calls)
        same_as(acc, r.stats(), want)
        assert np.array_equal(r.read_rng()["n"].reshape(-1), np.asarray(want[1])["n"].reshape(-1))
    finally:
        r.close()


@pytest.mark.parametrize("q_shift", [None, "3"])
@pytest.mark.parametrize("scene", ["DarkCornell", "lamp_box"])
def test_moments_of_batches_without_nee(monkeypatch, hipmod, oracle, rpt, world, scene, q_shift):
    """rpt_set_moments on: k_complete_moments adds every finished sample — the zeros of a HIT_DONE_ZERO slot included, they count — to the moments record.
    Batches of 5, 8 and 16 samples against the restatement fed with the oracle's per-sample radiances."""
    layout(monkeypatch, q_shift)
    w, view = the_scene(rpt, world, scene)
    cfg = rpt.default_config(W0, H0, nee=0, min_bounces=3, max_bounces=4, **view)
    if ("moments", scene) not in _cache:
        _cache[("moments", scene)] = ref.SampleBank(oracle, cfg, w, rpt.blue_noise_seeds(W0, H0))
    bank = _cache[("moments", scene)]
    batches = (5, 8, 16)
    total = sum(batches)
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w); r.set_config(cfg); r.reset(bank.rng(0))
        r.set_moments(True)
        for n in batches:
            r.render_async(n)
        r.wait()
        mom, want = r.read_moments(), bank.moments(total)
        assert ref.same_bits(mom, want), f"{int((mom.view(np.uint32) != want.view(np.uint32)).sum())} moments words differ"
        assert np.all(mom[..., 2] == total) and (mom[..., 3] == 0).any() and (mom[..., 3] > 0).any()      # pixels whose samples all ended with nothing, and others
        acc, n = r.read_accum()
        st = r.stats()
        assert n == total and ref.same_bits(acc, bank.accum(total))
        assert {k: st[k] for k in ref.STAT_KEYS} == bank.ray_counts(total)
    finally:
        r.close()


def lamp_box_with(rpt, emission, albedo0=None):
    """the lamp box with another emission, and optionally another albedo of material 0 (floor and ceiling).  The materials are changed after the world is
    built: its light table, which only NEE reads, still describes the emission it was built with."""
    w = seam.lamp_box_scene(rpt, False)
    w.materials["emissive"][3] = emission
    if albedo0 is not None:
        w.materials["albedo"][0] = albedo0
    return w


@pytest.mark.parametrize("q_shift", [None, "3"])
@pytest.mark.parametrize("case", ["emission (0, 5, 0)", "NaN albedo channel"])
def test_zero_signs_and_masked_terms(monkeypatch, hipmod, oracle, rpt, case, q_shift):
    """Emission (0, 5, 0): the term throughput x emission has zero channels, and 0 + term must give the bits that loading a zero record and adding gave.
    With a NaN in the red albedo of floor and ceiling every path that bounced there carries a NaN throughput: its term NaN x 0 is not finite, mask_nan3
    zeroes all of it, and the path still ends on the emitter's front — a record of zeros with HIT_DONE beside the HIT_DONE_ZERO of its neighbours.  (The few
    rays that slip out between the walls reach the sky, whose term is not masked: those pixels are NaN in the oracle's image too, and compared as NaN.)"""
    layout(monkeypatch, q_shift)
    nan = float("nan")
    w = lamp_box_with(rpt, [0.0, 5.0, 0.0, 1.0], [nan, 0.8, 0.8, 1.0] if case == "NaN albedo channel" else None)
    cfg = rpt.default_config(W0, H0, nee=0, min_bounces=3, max_bounces=4, **seam.LAMP_VIEW)
    seeds = rpt.blue_noise_seeds(W0, H0)
    want = oracle_image(oracle, ("signs", case), cfg, w, seeds, 16)
    green = want[0][..., 1]
    assert (green > 0).sum() > 1000                                       # the lamp is seen and found
    if case == "NaN albedo channel":
        clean = oracle_image(oracle, ("signs", "emission (0, 5, 0)"), cfg, lamp_box_with(rpt, [0.0, 5.0, 0.0, 1.0]), seeds, 16)
        assert (green < clean[0][..., 1]).sum() > 1000                    # terms were masked: the case is fit for the purpose
    acc, st, _, last_walk = seam._render(hipmod, w, cfg, seeds, (8, 8))
    assert last_walk
    same_as(acc, st, want)
