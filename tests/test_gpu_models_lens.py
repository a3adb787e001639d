"""Material models UNDER a camera lens on the device (rpt_set_material_models with rpt_set_camera_lens): accumulators, rng and counters word for word against
the restatement that carries both switches (tests/models_oracle models_lens_trace_cpu, held from both sides in tests/test_models_lens.py).  Each switch is
proven alone in tests/test_gpu_material_models.py and tests/test_gpu_camera_lens.py; here the two meet where the code composes them: k_shade_models behind
the FIRST walk over prepared slots ("fov") and behind the plain walk at bounce 0 (an aperture), slots restarted by k_lens_complete* and then shaded by
k_shade_models, the LAST walk that skips the shade stage, two slots per pixel forced by the lens with the models' variants and slot layouts.
80 x 72 (a whole tile, a 16-pixel and an 8-pixel remainder), 8 spp unless stated.

Which walks a case takes depends on where the scene lives: model_scenes' room, open scene and furnace (320-triangle spheres) are walked from global memory,
"textured" and "small_room" live in LDS — there iteration 0 under "fov" is the FIRST walk and a known-length batch without NEE ends in the LAST walk.  The
call-shape cases therefore run on the room AND on the small room.

The dimension budget (model_scenes.APERTURE_OVERRIDES): "fov" renders under the 31-dimension configurations of model_scenes.CONFIGS — the path reads table
entry 31, the lens does not —, "aperture" and "both" under 30 (no NEE) and 24 (NEE) dimensions."""
import os

import numpy as np
import pytest

import adaptive_ref
import guides_glass_ref
import lens_ref
import model_scenes
import moments_ref
from lens_ref import F

pytestmark = pytest.mark.gpu

W, H, SPP = 80, 72, 8
LENS_NAMES = ["fov", "aperture", "both"]


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


def counters_match(gs, st):
    got = (gs["extension_rays"], gs["shadow_rays"], gs["sky_evals"], gs["shadow_rays_elided"])
    want = (st.extension_rays, st.shadow_rays, st.sky_evals, st.shadow_rays_zero_term)
    assert got == want, (got, want)


def reference(oracle, name, nee, lens_name, spp=SPP, records=True):
    return model_scenes.reference(oracle, name, nee, W, H, spp, lens=lens_name, records=records, **model_scenes.lens_overrides(nee, lens_name))


class knobs:
    """the developer knobs of `env` in the environment for the length of the block; a value of None takes the variable out"""

    def __init__(self, env):
        self.env = env or {}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        for k, v in self.env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def create(hipmod, env=None, partition=None):
    """a Renderer created under the given knobs.  rpt_create reads them, and rpt_upload_scene reads those that act at upload (RPT_NO_LDS_SCENE,
    RPT_LAST_ORDER) AGAIN: prepare() uploads under the same environment"""
    with knobs(env):
        r = hipmod.Renderer(0) if partition is None else hipmod.Renderer(0, *partition)
    r.knobs = env
    return r


_contexts = {}


@pytest.fixture(scope="module")
def contexts(hipmod):
    """one context per (RPT_SHADE_COMPACT, RPT_SLOT_Q_SHIFT, RPT_NO_LDS_SCENE), shared by the tests of this file"""
    def get(compact=0, q_shift=None, no_lds=False):
        key = (compact, q_shift, no_lds)
        if key not in _contexts:
            _contexts[key] = create(hipmod, {"RPT_SHADE_COMPACT": str(compact), "RPT_SLOT_Q_SHIFT": q_shift, "RPT_NO_LDS_SCENE": "1" if no_lds else None})
        return _contexts[key]
    yield get
    for r in _contexts.values():
        r.close()
    _contexts.clear()


def prepare(r, rpt, name, nee, lens_name, records=True, lens_first=False):
    """scene, records, configuration, lens, reset.  The lens is taken off first: a context that still holds an aperture refuses a 31-dimension configuration"""
    w, rec, skybox, _ = model_scenes.scene(name)
    r.set_camera_lens(None)
    with knobs(getattr(r, "knobs", None)):
        r.upload_scene(w, skybox_f32=skybox)                  # (clears the records)
    r.set_config(model_scenes.config(name, nee, W, H, **model_scenes.lens_overrides(nee, lens_name)))
    if lens_first:
        r.set_camera_lens(lens_ref.lens(lens_name))
    if records:
        r.set_material_models(rec)
    if not lens_first:
        r.set_camera_lens(lens_ref.lens(lens_name))
    r.reset(rpt.blue_noise_seeds(W, H))


def check_against(r, ref, spp=SPP, counters=True):
    acc, rng, st = ref
    got, n = r.read_accum()
    assert n == spp and same_words(got, acc), f"{int((got.view(np.uint32) != acc.view(np.uint32)).any(-1).sum())} pixels differ"
    assert np.array_equal(r.read_rng().reshape(-1), np.asarray(rng).reshape(-1))
    if counters:
        counters_match(r.stats(), st)


@pytest.mark.parametrize("lens_name", LENS_NAMES)
@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("name", ["room", "small_room", "open", "textured"])
def test_words_and_counters_are_the_restatements(contexts, rpt, oracle, name, nee, lens_name):
    """the full cross.  In LDS (small_room, textured) under "fov": iteration 0 is the FIRST walk over prepared slots — the walk that starts no path meets
    k_shade_models —, under "aperture" and "both": k_generate_lens scatters the origins and bounce 0 takes the plain walk"""
    r = contexts()
    prepare(r, rpt, name, nee, lens_name)
    r.render(SPP)                                        # a batch of known length: no slot takes a second sample
    check_against(r, reference(oracle, name, nee, lens_name))


@pytest.mark.parametrize("lens_name", LENS_NAMES)
@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("name", ["room", "small_room"])
def test_walked_from_global_memory(contexts, rpt, oracle, name, nee, lens_name):
    """RPT_NO_LDS_SCENE=1: the global-memory walks (the room takes them anyway; the small room, which lives in LDS, takes them by the knob alone)"""
    r = contexts(no_lds=True)
    prepare(r, rpt, name, nee, lens_name)
    assert r.last_bounce_order()["mode"] == 0             # no LDS image is walked
    r.render(SPP)
    check_against(r, reference(oracle, name, nee, lens_name))


@pytest.mark.parametrize("lens_name", ["fov", "both"])
@pytest.mark.parametrize("nee", [0, 1])
@pytest.mark.parametrize("compact,q_shift", [(1, None), (0, "2"), (1, "2")])
@pytest.mark.parametrize("name", ["room", "small_room"])
def test_both_shade_variants_and_both_slot_layouts(contexts, rpt, oracle, name, compact, q_shift, nee, lens_name):
    """RPT_SHADE_COMPACT 0 / 1 and RPT_SLOT_Q_SHIFT unset / 2 ((0, unset) is every other test of this file)"""
    r = contexts(compact, q_shift)
    prepare(r, rpt, name, nee, lens_name)
    r.render(SPP)
    check_against(r, reference(oracle, name, nee, lens_name))


@pytest.mark.parametrize("lens_name", ["fov", "both"])
def test_the_last_walk_skips_the_shade_stage_under_lens_starts(hipmod, rpt, oracle, lens_name):
    """a known-length batch without NEE in an LDS scene (the small room): the last iteration's walk ends the paths itself — the surface rule "dead at the
    last bounce", which holds for every model — so a batch of max_bounces = 8 walks launches seven shade passes; words and counters are the restatement's
    all the same.  The room itself is walked from global memory, where all eight are launched."""
    r = create(hipmod, {"RPT_LAST_ORDER": None, "RPT_SLOT_Q_SHIFT": None, "RPT_NO_LDS_SCENE": None})
    try:
        prepare(r, rpt, "room", 0, lens_name)
        assert r.last_bounce_order()["mode"] == 0
        before = r.stats()["kernel_launches"]
        r.render(SPP)
        assert r.stats()["kernel_launches"]["shade"] - before["shade"] == 8
        check_against(r, reference(oracle, "room", 0, lens_name))
        prepare(r, rpt, "small_room", 0, lens_name)
        assert r.last_bounce_order()["mode"] != 0         # the small room lives in LDS and the LAST walk is on
        before = r.stats()["kernel_launches"]
        r.render(SPP)
        after = r.stats()["kernel_launches"]
        d = {k: after[k] - before[k] for k in after}
        print("launches of the batch:", d)
        assert d["traverse"] == 8 and d["shade"] == 7 and d["generate"] == 1 and d["complete"] == 1 and d["shadow"] == 0
        check_against(r, reference(oracle, "small_room", 0, lens_name))
    finally:
        r.close()


@pytest.mark.parametrize("name", ["room", "small_room"])
@pytest.mark.parametrize("q_shift", [None, "2"])
def test_slots_that_take_several_samples(hipmod, rpt, oracle, q_shift, name):
    """20 spp with 4 samples in flight, polled: k_lens_complete restarts the finished slots and k_shade_models shades what it started"""
    r = create(hipmod, {"RPT_SLOT_Q_SHIFT": q_shift})
    try:
        r.set_samples_in_flight(4)
        prepare(r, rpt, name, 1, "both")
        r.render(20)
        check_against(r, reference(oracle, name, 1, "both", 20), 20)
    finally:
        r.close()


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_two_batches_and_an_asynchronous_one(contexts, rpt, oracle, name):
    r = contexts()
    prepare(r, rpt, name, 1, "both")
    r.render(3)
    r.render(5)
    check_against(r, reference(oracle, name, 1, "both"))
    r.reset(rpt.blue_noise_seeds(W, H))
    r.render_async(SPP)
    r.wait()
    check_against(r, reference(oracle, name, 1, "both"))


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_a_one_sample_call_uses_slot_0_of_2(hipmod, rpt, oracle, name):
    r = create(hipmod)
    try:
        r.set_samples_in_flight(2)
        prepare(r, rpt, name, 1, "both")
        r.render(1)
        check_against(r, reference(oracle, name, 1, "both", 1), 1)
    finally:
        r.close()


@pytest.mark.parametrize("name", ["room", "small_room"])
@pytest.mark.parametrize("in_flight,spp", [(None, SPP), (2, 5)])
def test_moments_on(hipmod, rpt, oracle, in_flight, spp, name):
    """k_lens_complete_moments, in one completion of a known-length batch and restarting slots (5 samples through 2 slots): the record is tests/moments_ref.py
    over the combined restatement's per-sample radiances"""
    samples = model_scenes.per_sample_radiances(oracle, name, 1, W, H, SPP, lens="both", **model_scenes.lens_overrides(1, "both"))
    want = np.zeros((H, W, 4), F)
    acc = np.zeros((H, W, 4), F)
    for k in range(spp):
        moments_ref.add_sample(want, samples[k])
        acc[..., :3] = acc[..., :3] + samples[k]
        acc[..., 3] = acc[..., 3] + F(1)
    r = create(hipmod)
    try:
        if in_flight is not None:
            r.set_samples_in_flight(in_flight)
        r.set_moments(True)
        prepare(r, rpt, name, 1, "both")
        r.render(spp)
        if spp == SPP:
            check_against(r, reference(oracle, name, 1, "both"))
        assert same_words(r.read_accum()[0], acc)
        assert same_words(r.read_moments(), want)
    finally:
        r.close()


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_masked_pass_over_a_checkerboard(hipmod, rpt, oracle, name):
    acc, rng, _ = reference(oracle, name, 1, "both")
    y, x = np.mgrid[0:H, 0:W]
    mask = (x + y) % 2 == 0
    r = create(hipmod)
    try:
        prepare(r, rpt, name, 1, "both")
        r.render_pixels(mask, SPP)
        got, _ = r.read_accum()
        assert same_words(got[mask], acc[mask]) and not got[~mask].any()
        assert np.array_equal(r.read_rng().reshape(H, W)[mask], np.asarray(rng).reshape(H, W)[mask])
    finally:
        r.close()


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_rank_one_of_three(hipmod, rpt, oracle, name):
    acc, _, _ = reference(oracle, name, 1, "both")
    xy = hipmod.tile_order(W, H, 1, 3)
    own = np.zeros((H, W), bool)
    own[xy >> 16, xy & 0xFFFF] = True
    r = create(hipmod, partition=(1, 3))
    try:
        prepare(r, rpt, name, 1, "both")
        r.render(SPP)
        got, _ = r.read_accum()
        assert own.any() and same_words(got[own], acc[own]) and not got[~own].any()
    finally:
        r.close()


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_three_ranks_on_one_device(hipmod, rpt, oracle, name):
    """rpt_multi_set_material_models and rpt_multi_set_camera_lens together: the gathered image is the restatement's, the counters sum to its"""
    acc, _, st = reference(oracle, name, 1, "both")
    w, rec, skybox, _ = model_scenes.scene(name)
    m = hipmod.MultiRenderer([0, 0, 0], allow_shared_device=True)
    try:
        m.upload_scene(w, skybox_f32=skybox)
        m.set_material_models(rec)
        m.set_config(model_scenes.config(name, 1, W, H, **model_scenes.lens_overrides(1, "both")))
        m.set_camera_lens(lens_ref.lens("both"))
        m.reset(rpt.blue_noise_seeds(W, H))
        m.render(SPP)
        got, n = m.read_accum()
        assert n == SPP and same_words(got, acc)
        counters_match(m.stats(), st)
    finally:
        m.close()


@pytest.mark.parametrize("compact", [0, 1])
def test_furnace_on_the_device_under_a_lens(contexts, rpt, oracle, compact):
    """every sample is exactly the sky's f32 value or 0, under "both" (the primary-miss mask of the reference camera is not asserted: the per-sample property)"""
    r = contexts(compact)
    prepare(r, rpt, "furnace", 0, "both")
    r.render(SPP)
    acc, n = r.read_accum()
    assert n == SPP
    k = model_scenes.furnace_check(acc, model_scenes.furnace_sky_value(oracle, W, H), None, SPP)
    assert (k == SPP).any()
    check_against(r, reference(oracle, "furnace", 0, "both"))


def _launches(r):
    return dict(r.stats()["kernel_launches"])


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_the_order_of_the_setters_does_not_matter(hipmod, rpt, oracle, name):
    """records before or after the lens: the same words, counters and kernel launches"""
    results = []
    for lens_first in (False, True):
        r = create(hipmod)
        try:
            prepare(r, rpt, name, 1, "both", lens_first=lens_first)
            r.render(SPP)
            check_against(r, reference(oracle, name, 1, "both"))
            results.append(_launches(r))
        finally:
            r.close()
    assert results[0] == results[1]


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_settings_changed_between_batches_and_taken_off(hipmod, rpt, oracle, name):
    """a lens set between two batches with a reset; rpt_set_camera_lens(NULL) with the records still set gives the models-only reference, kernel launches
    included (those of a context that never set a lens); records cleared under the lens give the lens-only image"""
    w, rec, skybox, _ = model_scenes.scene(name)
    more = model_scenes.lens_overrides(1, "both")
    models_only = model_scenes.reference(oracle, name, 1, W, H, SPP, **more)
    never = create(hipmod)
    try:
        never.upload_scene(w, skybox_f32=skybox)
        never.set_material_models(rec)
        never.set_config(model_scenes.config(name, 1, W, H, **more))
        never.reset(rpt.blue_noise_seeds(W, H))
        before = _launches(never)
        never.render(SPP)
        check_against(never, models_only)
        never_launches = {k: v - before[k] for k, v in _launches(never).items()}
    finally:
        never.close()
    r = create(hipmod)
    try:
        prepare(r, rpt, name, 1, None)                  # records, no lens
        assert more and r.camera_lens().aperture_radius == 0.0
        r.set_config(model_scenes.config(name, 1, W, H, **more))
        r.reset(rpt.blue_noise_seeds(W, H))
        r.render(SPP)
        check_against(r, models_only)
        r.set_camera_lens(lens_ref.lens("both"))          # the lens arrives between two batches ...
        r.reset(rpt.blue_noise_seeds(W, H))
        r.render(SPP)
        check_against(r, reference(oracle, name, 1, "both"))
        r.set_camera_lens(lens_ref.lens("fov"))           # ... changes ...
        r.reset(rpt.blue_noise_seeds(W, H))
        r.render(SPP)
        check_against(r, model_scenes.reference(oracle, name, 1, W, H, SPP, lens="fov", **more))
        r.set_camera_lens(None)                           # ... and leaves, the records still set
        assert np.array_equal(r.material_models(), rec)
        r.reset(rpt.blue_noise_seeds(W, H))
        before = _launches(r)
        r.render(SPP)
        check_against(r, models_only)
        assert {k: v - before[k] for k, v in _launches(r).items()} == never_launches
        r.set_camera_lens(lens_ref.lens("both"))
        r.set_material_models(None)                       # the records leave under the lens: the lens restatement's image (every record PBR)
        r.reset(rpt.blue_noise_seeds(W, H))
        r.render(SPP)
        check_against(r, reference(oracle, name, 1, "both", records=False))
    finally:
        r.close()


def test_an_aperture_with_31_dimensions_is_refused_with_records_set(hipmod, rpt):
    """whichever of rpt_set_config / rpt_set_camera_lens comes second (RPT_ECONFIG, -4), as tests/test_gpu_camera_lens.py has it without records; the context
    keeps what it had"""
    r = create(hipmod)
    try:
        for nee in (0, 1):
            prepare(r, rpt, "room", nee, "both")
            with pytest.raises(hipmod.RptError) as e:                                     # the configuration comes second
                r.set_config(model_scenes.config("room", nee, W, H))
            assert e.value.code == -4 and "31" in str(e.value) and "rpt_set_config" in str(e.value)
            r.render(2)                                                                   # ... and the context renders on
            r.set_camera_lens(lens_ref.lens("fov"))
            r.set_config(model_scenes.config("room", nee, W, H))                          # no aperture: 31 dimensions are the configuration's
            for name in ("both", "aperture"):
                with pytest.raises(hipmod.RptError) as e:                                 # the lens comes second
                    r.set_camera_lens(lens_ref.lens(name))
                assert e.value.code == -4 and "31" in str(e.value) and "rpt_set_camera_lens" in str(e.value)
            now = r.camera_lens()
            assert (now.tan_half_fov, now.aperture_radius) == (float(F(lens_ref.LENSES["fov"][0])), 0.0)
            assert np.array_equal(r.material_models(), model_scenes.scene("room")[1])
    finally:
        r.close()


# ---- everything on at once -------------------------------------------------------------------------------------------------------------------------------
MASK_SPP, FULL_SPP = 3, 5


def coarse_checkerboard():
    """cells of 5 x 4 pixels, every other one: a mask made of rectangles, so that the restatement's counters of the masked pass are sums over rectangles"""
    y, x = np.mgrid[0:H, 0:W]
    mask = (x // 5 + y // 4) % 2 == 0
    rects = [(x0, y0, x0 + 5, y0 + 4) for y0 in range(0, H, 4) for x0 in range(0, W, 5) if (x0 // 5 + y0 // 4) % 2 == 0]
    return mask, rects


_everything = {}


def everything_reference(oracle, rpt, name):
    """a masked pass of MASK_SPP samples followed by a full pass of FULL_SPP under records + "both" with MIS: accumulator and moments from the combined
    restatement's sample bank (a masked pixel takes samples 0 .. 7, another 0 .. 4), rng by the counts, counters as sums of the restatement's over the
    mask's rectangles and then over the image, chained through the rng"""
    if name not in _everything:
        more = model_scenes.lens_overrides(1, "both")
        mask, rects = coarse_checkerboard()
        bank = model_scenes.per_sample_radiances(oracle, name, 1, W, H, MASK_SPP + FULL_SPP, lens="both", **more)
        acc, mom = np.zeros((H, W, 4), F), np.zeros((H, W, 4), F)
        for k in range(MASK_SPP + FULL_SPP):
            sample = bank[k] if k < MASK_SPP else np.where(mask[..., None], bank[k], bank[k - MASK_SPP])
            new_acc, new_mom = acc.copy(), mom.copy()
            new_acc[..., :3] = new_acc[..., :3] + sample
            new_acc[..., 3] = new_acc[..., 3] + F(1)
            moments_ref.add_sample(new_mom, sample)
            take = mask if k < MASK_SPP else np.ones_like(mask)
            acc[take], mom[take] = new_acc[take], new_mom[take]
        w, rec, skybox, _ = model_scenes.scene(name)
        cfg, sc = model_scenes.config(name, 1, W, H, **more), oracle.scene(w, skybox_f32=skybox)
        rng = rpt.blue_noise_seeds(W, H)
        total = np.zeros(4, np.int64)
        for rect in rects:
            _, rng, st = model_scenes.models_lens_trace_cpu(cfg, sc, rec, lens_ref.lens("both"), rng, MASK_SPP, rect=rect, threads=1)
            total += (st.extension_rays, st.shadow_rays, st.sky_evals, st.shadow_rays_zero_term)
        _, rng, st = model_scenes.models_lens_trace_cpu(cfg, sc, rec, lens_ref.lens("both"), rng, FULL_SPP)
        total += (st.extension_rays, st.shadow_rays, st.sky_evals, st.shadow_rays_zero_term)
        guides, info = guides_glass_ref.guides(w, rec, 2, cfg, oracle, sc, rays=lens_ref.centre_rays(cfg, lens_ref.LENSES["both"][0], oracle))
        _everything[name] = dict(mask=mask, acc=acc, moments=mom, rng=rng, counters=tuple(int(v) for v in total), guides=guides, info=info, cfg=cfg)
    return _everything[name]


def everything_on(r, rpt, name):
    prepare(r, rpt, name, 1, "both")
    r.set_moments(True)
    r.set_guides_through_glass(2)
    assert r.shadow_mode() == 0                           # SEGMENT off
    r.reset(rpt.blue_noise_seeds(W, H))
    r.render_pixels(coarse_checkerboard()[0], MASK_SPP)
    r.render(FULL_SPP)


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_everything_on_at_once_on_one_context(hipmod, rpt, oracle, name):
    """records, "both", guides through glass K = 2, moments — a masked pass, then a full pass: accumulator, rng, counters and the moments record are the
    combined restatement's, the guides the CPU chain's over the lens-centre rays, rpt_denoise_variance with the firefly clamp its host build over them"""
    want = everything_reference(oracle, rpt, name)
    r = create(hipmod)
    try:
        everything_on(r, rpt, name)
        got, _ = r.read_accum()
        assert same_words(got, want["acc"]), f"{int((got.view(np.uint32) != want['acc'].view(np.uint32)).any(-1).sum())} pixels differ"
        assert np.array_equal(r.read_rng().reshape(-1), np.asarray(want["rng"]).reshape(-1))
        gs = r.stats()
        assert (gs["extension_rays"], gs["shadow_rays"], gs["sky_evals"], gs["shadow_rays_elided"]) == want["counters"]
        moments = r.read_moments()
        assert same_words(moments, want["moments"]) and not r.counts_uniform()
        g = r.guides()
        for plane in ("albedo", "normal", "depth", "position", "kind"):
            assert np.array_equal(np.ascontiguousarray(g[plane]).view(np.uint32), np.ascontiguousarray(want["guides"][plane]).view(np.uint32)), plane
        info = r.guides_info()
        assert info["max_interfaces"] == 2 and all(info[k] == want["info"][k] for k in ("rounds", "rays", "pixels_through_glass", "pixels_exhausted"))
        assert want["info"]["pixels_through_glass"] > 0
        cg = want["guides"]
        mean = (want["acc"][..., :3] / want["acc"][..., 3:]).astype(F)
        tan_half = F(lens_ref.LENSES["both"][0])
        fields = dict(iterations=3, sigma_variance=4.0, clamp_scale=2.0, clamp_radius=2)
        vp = hipmod.denoise_var_params(sigma_plane=1.0, **fields)
        rgb, var, rep = r.denoise_variance(params=vp, with_report=True)
        host = hipmod.denoise_variance_host(mean, cg["albedo"], cg["normal"], cg["position"], cg["depth"], cg["kind"], want["moments"],
                                            hipmod.denoise_var_params(sigma_plane=float(F(1.0) * tan_half), **fields), 0)
        for a, b in ((rgb, host[0]), (var, host[1])):
            na, nb = np.isnan(a), np.isnan(b)
            assert np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))
        clamped = hipmod.firefly_host(mean, cg["albedo"], cg["kind"], want["moments"], want["acc"][..., 3].copy(), 0, vp.clamp_scale, vp.clamp_floor, vp.clamp_radius,
                                      vp.base.iterations != 0 and vp.base.demodulate != 0)[2] != 0
        print(f"{name}: pixels_clamped {rep['pixels_clamped']}")
        assert rep["pixels_clamped"] == int(clamped.sum())
    finally:
        r.close()


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_everything_on_at_once_on_rank_one_of_three(hipmod, rpt, oracle, name):
    """the same two passes on rank 1 of 3: its own pixels carry the restatement's accumulator, rng and moments, the others nothing"""
    want = everything_reference(oracle, rpt, name)
    xy = hipmod.tile_order(W, H, 1, 3)
    own = np.zeros((H, W), bool)
    own[xy >> 16, xy & 0xFFFF] = True
    r = create(hipmod, partition=(1, 3))
    try:
        everything_on(r, rpt, name)
        got, _ = r.read_accum()
        assert own.any() and same_words(got[own], want["acc"][own]) and not got[~own].any()
        assert np.array_equal(r.read_rng().reshape(H, W)[own], np.asarray(want["rng"]).reshape(H, W)[own])
        assert same_words(r.read_moments()[own], want["moments"][own])
    finally:
        r.close()


# ---- to a noise target -----------------------------------------------------------------------------------------------------------------------------------
class handed_restatement:
    """what tests/moments_ref.py SampleBank asks of the oracle it is handed — scene() and trace_cpu() — over the combined restatement: the bank and
    tests/adaptive_ref.py stay as they are"""

    def __init__(self, oracle, records, lens_record):
        self.oracle, self.records, self.lens_record = oracle, records, lens_record

    def scene(self, world, skybox_f32=None):
        return self.oracle.scene(world, skybox_f32=skybox_f32)

    def trace_cpu(self, cfg, scene, rng, n_samples):
        return model_scenes.models_lens_trace_cpu(cfg, scene, self.records, self.lens_record, rng, n_samples)


@pytest.mark.parametrize("name", ["room", "small_room"])
def test_adaptive_run_to_a_noise_target(hipmod, rpt, oracle, name):
    """rpt_render_adaptive under records + "both", MIS: min 8, batch 8, max 32, threshold 0.3 — per-pixel counts, accumulator, rng, moments, passes and the
    counts are tests/adaptive_ref.py's prediction from the combined restatement's sample bank, exactly.  (Confirmed from the bank before the parameters
    were committed: about 4 800 pixels stop at 8, 250 reach the cap, all four counts of the schedule occur.)"""
    w, rec, skybox, _ = model_scenes.scene(name)
    cfg = model_scenes.config(name, 1, W, H, **model_scenes.lens_overrides(1, "both"))
    bank = moments_ref.SampleBank(handed_restatement(oracle, rec, lens_ref.lens("both")), cfg, w, rpt.blue_noise_seeds(W, H), skybox_f32=skybox)
    t = adaptive_ref.Target(0.3, 0, 8, 8, 32)
    sim = adaptive_ref.simulate(bank, t)
    n = sim["counts_image"]
    print(f"{name}: predicted {sim['passes']} passes, converged {sim['converged']}, {sim['pixel_samples']} pixel-samples, pixels per count "
          f"{dict(zip(*[a.tolist() for a in np.unique(n, return_counts=True)]))}")
    assert len(np.unique(n)) == 4 and np.array_equal(n, adaptive_ref.closed_form(bank, t))          # the prediction itself is not trivial
    want_acc, want_rng, want_mom = adaptive_ref.expected_state(bank, n)
    r = create(hipmod)
    try:
        prepare(r, rpt, name, 1, "both")
        res = r.render_adaptive(**t.kwargs())
        assert r.moments_on() and not r.counts_uniform()
        got, _ = r.read_accum()
        assert np.array_equal(got[..., 3], n.astype(F))
        assert same_words(got, want_acc), f"{int((got.view(np.uint32) != want_acc.view(np.uint32)).any(-1).sum())} pixels differ"
        assert np.array_equal(r.read_rng().reshape(H, W), want_rng)
        assert same_words(r.read_moments(), want_mom)
        assert (res["passes"], res["converged"], res["counts"], res["pixel_samples"]) == (sim["passes"], sim["converged"], sim["counts"], sim["pixel_samples"])
        assert r.stats()["samples"] == sim["pixel_samples"]
    finally:
        r.close()
