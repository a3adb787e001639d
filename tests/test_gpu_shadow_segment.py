"""RPT_SHADOW_SEGMENT on the device (rpt.h rpt_set_shadow_mode; the rule: tests/test_shadow_segment.py).  Ray level: the bounded any-hit walk of the
test hook answers `.hit` as the CPU model of the rule does, bit for bit.  Image level, through the production kernels — every `_seg` instantiation a
scene or a developer knob reaches: per-pixel relative L2 against the oracle < 1e-4 (BASELINE.md's contract; SEGMENT is outside the bit-for-bit one), ray
counts equal to the exact run's, and the number of accumulator words that differ from the exact image of the same context recorded (expected 0, not
asserted; kept copy: profiles/r10_shadow_segment_parity.txt, rewritten by a full run with RPT_PROFILE_DIR=profiles).  Plumbing: default, switching, the multi-GPU driver, invalid modes, nee = 0."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_ffi import _p  # noqa: E402
from test_anyhit_order import _shadow_like_rays  # noqa: E402

pytestmark = pytest.mark.gpu

L2_BOUND = 1e-4           # per-pixel relative L2 error vs the CPU path
RECORD = []               # lines of profiles/r10_shadow_segment_parity.txt


@pytest.fixture(scope="module", autouse=True)
def parity_record():
    """The record is printed by every case; it is written to a file only where RPT_PROFILE_DIR names a directory (profiles/ to refresh the kept copy) and
    only when every image case ran, so that a partial run never replaces the full record."""
    yield
    d = os.environ.get("RPT_PROFILE_DIR")
    if d and len([line for line in RECORD if not line.startswith(" ")]) == len(CASES):
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "r10_shadow_segment_parity.txt"), "w") as f:
            f.write("# tests/test_gpu_shadow_segment.py: RPT_SHADOW_SEGMENT against RPT_SHADOW_EXACT on one context, and against the oracle on two windows\n")
            f.write("# case | accumulator words that differ from the EXACT image (whole image) | worst per-pixel relative L2 vs the oracle in the windows | shadow rays (elided)\n")
            f.write("\n".join(RECORD) + "\n")


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    so = tmp_path_factory.mktemp("segment") / "libanyhit_sim.so"
    subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-msse4.1", "-pthread", "-shared", "-o", str(so),
                    os.path.join(ROOT, "tools", "anyhit_order_sim.cpp")], check=True)
    return C.CDLL(str(so))


_scenes = {}


def _world(world, name):
    if name not in _scenes:
        import scenes
        if name == "deep_bvh_1m":
            _scenes[name] = scenes.deep_bvh_scene(1_000_000)
        elif name == "scatter":
            _scenes[name] = scenes.scatter_scene(80_000)
        elif name == "scatter_deep":
            _scenes[name] = scenes.scatter_scene(300_000)
        elif name == "foreign_pool":
            _scenes[name] = scenes.foreign_pool(scenes.scatter_scene())
        else:
            _scenes[name] = world(name)
    return _scenes[name]


def worst_pixel_rel_l2(got, ref):
    """max over the pixels of |got - ref| / |ref| (rgb); a pixel the reference leaves black or non-finite has to be the reference's exactly"""
    g = got[..., :3].reshape(-1, 3).astype(np.float64)
    r = ref[..., :3].reshape(-1, 3).astype(np.float64)
    den = np.linalg.norm(r, axis=1)
    plain = np.isfinite(r).all(axis=1) & (den > 0)
    assert np.array_equal(g[~plain], r[~plain], equal_nan=True)
    return float((np.linalg.norm(g[plain] - r[plain], axis=1) / den[plain]).max()) if plain.any() else 0.0


# ---- ray level

@pytest.mark.parametrize("scene", ["DarkCornell", "VeachMIS", "FurnaceTest", "PBRTest"])
def test_the_hooks_bounded_walk_is_the_cpu_models(renderer, sim, oracle, world, scene):
    w = world(scene)
    sc = oracle.scene(w)
    rng = np.random.default_rng(41)
    n = 250_000
    o, d, max_t = _shadow_like_rays(rng, n, w)
    model = np.zeros(n, np.uint8)
    sim.sim_any_hit_segment(C.byref(sc), C.c_size_t(n), _p(o), _p(d), _p(max_t), 0, C.c_uint32(0), _p(model))
    ref = np.zeros(n, np.uint8)
    sim.sim_any_hit_order(C.byref(sc), C.c_size_t(n), _p(o), _p(d), _p(max_t), 0, C.c_uint32(0), _p(ref))
    renderer.upload_scene(w)
    _, _, flags = renderer.debug_trace_rays(2, o, d, max_t)
    hit = (flags & 1).astype(np.uint8)
    print(f"{scene}: {int(hit.sum())} occluded of {n}; differ from the model {int((hit != model).sum())}, from the reference's walk {int((hit != ref).sum())}")
    assert np.array_equal(hit, model), int((hit != model).sum())
    assert np.array_equal(model, ref)                      # (tests/test_shadow_segment.py: no loss on these rays) and so the device's answer is the oracle's
    _, _, exact = renderer.debug_trace_rays(1, o, d, max_t)
    assert np.array_equal((exact & 1).astype(np.uint8), ref)


def test_the_hooks_bounded_walk_on_rays_without_a_bound(renderer, world):
    """max_t >= 1e6 is the exact walk; NaN accepts nothing; max_t <= 0 accepts nothing (t > 0.001)"""
    w = world("DarkCornell")
    rng = np.random.default_rng(3)
    n = 30_000
    o, d, _ = _shadow_like_rays(rng, n, w)
    renderer.upload_scene(w)
    for bound in (1e6, 2e6, np.inf, np.nan, 0.0, -0.0, -1.0, 1e-45, -np.inf):
        max_t = np.full(n, bound, np.float32)
        a = renderer.debug_trace_rays(1, o, d, max_t)[2] & 1
        b = renderer.debug_trace_rays(2, o, d, max_t)[2] & 1
        assert np.array_equal(a, b), bound
        assert (a.sum() > 0) == bool(bound >= 1e6), bound


# ---- image level: the production kernels

FULL = [("DarkCornell", 1024, 1024, 32, {}), ("VeachMIS", 1920, 1080, 32, {})]
CASES = [(s, W, H, spp, nee, over, {"RPT_SHADOW_ORDER": order}) for (s, W, H, spp, over) in FULL for nee in (1, 2) for order in ("near", "fixed")]
CASES += [("deep_bvh_1m", 512, 512, 8, 1, {"cam_position": (0.0, 2.5, -0.5, 0.0)}, {"RPT_SHADOW_ORDER": order}) for order in ("near", "fixed")]
CASES += [("DarkCornell", 1024, 1024, 32, 1, {}, env) for env in ({"RPT_NO_LDS_SCENE": "1"}, {"RPT_COOP_LEAVES": "1"}, {"RPT_STACK_BITS": "21"}, {"RPT_STACK_BITS": "24"},
                                                                 {"RPT_STACK_BITS": "32"})]
# DarkCornell's tree is shallow (16-entry stacks, 16-bit entries whatever RPT_STACK_BITS says) and lives in LDS (no cooperative leaves): the instantiations those
# knobs are about are reached by walking it from global memory with the cooperative build, by deep trees with every entry width, and by a foreign node pool
CASES += [("DarkCornell", 256, 256, 8, 1, {}, {"RPT_NO_LDS_SCENE": "1", "RPT_COOP_LEAVES": "1", "RPT_SHADOW_ORDER": order}) for order in ("near", "fixed")]
CASES += [(s, 128, 96, 4, 1, {"cam_position": (0.0, 1.8, -0.9, 0.0)}, {"RPT_STACK_BITS": bits, "RPT_COOP_LEAVES": coop, "RPT_SHADOW_ORDER": order})
          for s in ("scatter", "scatter_deep") for bits in ("16", "21", "24", "32") for (coop, order) in (("0", "near"), ("1", "fixed"))]
CASES += [("foreign_pool", 128, 96, 4, 1, {"cam_position": (0.0, 1.8, -0.9, 0.0)}, {})]


def _case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-nee{c[4]}-" + ("_".join(f"{k[4:].lower()}={v}" for k, v in c[6].items()) or "default")


def _cpu_lost_occlusions(sim, cfg, sc, seeds, pixels, spp):
    """{x | y << 16: [(sample, bounce), ...]}: the shadow rays the device walks for the first spp samples of these pixels (the oracle's trace_pixel dumps them) that
    the reference's walk calls occluded and the CPU model of the segment rule does not"""
    pix = np.array(pixels, np.uint32)
    n = len(pix)
    lost = {}
    for s in range(spp):
        for bounce in range(cfg.max_bounces):
            rays = np.zeros((n, 8), np.float32)
            valid = np.zeros(n, np.uint8)
            sim.sim_dump_shadow_rays(C.byref(cfg), C.byref(sc), _p(seeds), C.c_uint32(s), C.c_uint32(bounce), _p(pix), C.c_size_t(n), _p(rays), _p(valid))
            sel = np.flatnonzero(valid == 1)
            if len(sel) == 0:
                continue
            o, d, max_t = np.ascontiguousarray(rays[sel, 0:3]), np.ascontiguousarray(rays[sel, 3:6]), np.ascontiguousarray(rays[sel, 6])
            exact, bounded = np.zeros(len(sel), np.uint8), np.zeros(len(sel), np.uint8)
            sim.sim_any_hit_order(C.byref(sc), C.c_size_t(len(sel)), _p(o), _p(d), _p(max_t), 0, C.c_uint32(0), _p(exact))
            sim.sim_any_hit_segment(C.byref(sc), C.c_size_t(len(sel)), _p(o), _p(d), _p(max_t), 0, C.c_uint32(0), _p(bounded))
            assert not ((bounded == 1) & (exact == 0)).any()
            for i in np.flatnonzero(exact != bounded):
                lost.setdefault(int(pix[sel[i]]), []).append((s, bounce))
    return lost


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_segment_images_hold_the_parity_contract(monkeypatch, sim, hipmod, oracle, rpt, world, case):
    """Asserted: the ray counts of the two modes are equal, and per-pixel relative L2 of the SEGMENT image against the oracle < 1e-4 on two windows.  Recorded:
    the accumulator words that differ between the two modes over the whole image.  Beyond that, a defect detector of this file's own: every pixel that differs
    must be one where the CPU model of the rule loses an occlusion too.  It finds the pixel's rays through sim_dump_shadow_rays — a second statement of which
    rays the shade stage queues — so if a legitimate loss ever fails here, suspect that selection before the kernels."""
    scene, W, H, spp, nee, over, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    w = _world(world, scene)
    cfg = rpt.default_config(W, H, nee=nee, **over)
    seeds = rpt.blue_noise_seeds(W, H)
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        if "RPT_SHADOW_ORDER" in env:
            assert r.shadow_order()["fixed"] == (env["RPT_SHADOW_ORDER"] == "fixed")
        r.set_config(cfg)
        images, stats = {}, {}
        for mode in (hipmod.SHADOW_EXACT, hipmod.SHADOW_SEGMENT):
            r.set_shadow_mode(mode)
            assert r.shadow_mode() == mode
            r.reset(seeds)
            r.render(spp)
            images[mode], s = r.read_accum()
            images[mode] = images[mode].copy()
            stats[mode] = r.stats()
            assert s == spp
    finally:
        r.close()
    ex, sg = images[hipmod.SHADOW_EXACT], images[hipmod.SHADOW_SEGMENT]
    differ = int((ex.view(np.uint32) != sg.view(np.uint32)).sum())
    se, ss = stats[hipmod.SHADOW_EXACT], stats[hipmod.SHADOW_SEGMENT]
    ww, wh = 48, 40
    sc = oracle.scene(w)
    worst = 0.0
    for (x0, y0) in ((W // 2 - ww // 2, H // 2 - wh // 2), (W - ww, H - wh)):
        ref, _, _ = oracle.trace_cpu(cfg, sc, seeds, spp, rect=(x0, y0, x0 + ww, y0 + wh))
        win = (slice(y0, y0 + wh), slice(x0, x0 + ww))
        assert np.array_equal(ex[win].view(np.uint32), ref[win].view(np.uint32)), (x0, y0)       # the exact mode is untouched: the oracle's window bit for bit
        worst = max(worst, worst_pixel_rel_l2(sg[win], ref[win]))
    line = f"{_case_id(case)} | {differ} of {ex.size} | {worst:.3e} | {ss['shadow_rays']} ({ss['shadow_rays_elided']})"
    print(line)
    RECORD.append(line)
    # Where the two images differ a shadow ray of that pixel answered differently — the rays themselves are the same in both modes (an NEE term only adds to the
    # radiance) — and the CPU model of the rule, the same arithmetic, has to lose an occlusion on a ray of that very pixel: a difference the rule does not
    # explain would be a defect of the kernels, whatever its size.
    where = np.argwhere((ex.view(np.uint32) != sg.view(np.uint32)).any(axis=2))
    if len(where):
        assert len(where) <= 64, len(where)
        lost = _cpu_lost_occlusions(sim, cfg, sc, seeds, [int(y) << 16 | int(x) for (y, x) in where], spp)
        for (y, x) in where:
            note = f"    pixel ({int(x)}, {int(y)}): exact {ex[y, x, :3].tolist()} segment {sg[y, x, :3].tolist()}; the CPU model loses (sample, bounce) {lost.get(int(y) << 16 | int(x))}"
            print(note)
            RECORD.append(note)
        assert all((int(y) << 16 | int(x)) in lost for (y, x) in where)
    assert se["shadow_rays"] > 0
    assert (ss["shadow_rays"], ss["shadow_rays_elided"], ss["extension_rays"]) == (se["shadow_rays"], se["shadow_rays_elided"], se["extension_rays"])
    assert worst < L2_BOUND, worst


# ---- image level, with the other opt-in settings: material models (rpt_set_material_models) and a camera lens (rpt_set_camera_lens)

# (scene, records, lens, nee): Lambertian and PBR next-event estimation through the `_seg` kernels — Glass queues no shadow ray —, from global memory (room,
# open: 320-triangle spheres) and from LDS (small_room, DarkCornell); shadow rays of paths that a lens started; both at once
COMBINED = [(scene, True, None, nee) for scene in ("room", "small_room", "open") for nee in (1, 2)]
COMBINED += [("DarkCornell", False, "both", nee) for nee in (1, 2)]
COMBINED += [(scene, True, "both", nee) for scene in ("room", "small_room") for nee in (1, 2)]


@pytest.mark.parametrize("scene,records,lens_name,nee", COMBINED, ids=lambda v: str(v))
def test_segment_with_material_models_and_a_lens(hipmod, oracle, rpt, world, scene, records, lens_name, nee):
    """The same contract as above at 80 x 72 x 8 spp, against the restatement that carries the switch (tests/models_oracle with both, tests/lens_oracle for
    DarkCornell) over the WHOLE image: ray counts equal to the exact run's — and the restatement's —, per-pixel relative L2 of the SEGMENT image < L2_BOUND;
    and the same context, switched back to EXACT and reset, gives the restatement bit for bit.  Printed: the accumulator words that differ between the modes."""
    import lens_ref
    import model_scenes
    W, H, spp = 80, 72, 8
    seeds = rpt.blue_noise_seeds(W, H)
    if scene == "DarkCornell":
        w, rec, skybox = world(scene), None, None
        cfg = lens_ref.config(world, scene, nee, W, H)
        ref, ref_rng, st = lens_ref.reference(oracle, world, scene, nee, lens_name, W, H, spp)
    else:
        w, rec, skybox, _ = model_scenes.scene(scene)
        more = model_scenes.lens_overrides(nee, lens_name)
        cfg = model_scenes.config(scene, nee, W, H, **more)
        ref, ref_rng, st = model_scenes.reference(oracle, scene, nee, W, H, spp, lens=lens_name, **more)
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w, skybox_f32=skybox)
        if records:
            r.set_material_models(rec)
        r.set_config(cfg)
        r.set_camera_lens(lens_ref.lens(lens_name))
        images, stats = {}, {}
        for mode in (hipmod.SHADOW_SEGMENT, hipmod.SHADOW_EXACT):          # EXACT last: what SEGMENT leaves behind
            r.set_shadow_mode(mode)
            assert r.shadow_mode() == mode
            r.reset(seeds)
            r.render(spp)
            images[mode], n = r.read_accum()
            images[mode] = images[mode].copy()
            stats[mode] = r.stats()
            assert n == spp
        rng_after = r.read_rng().copy()
    finally:
        r.close()
    ex, sg = images[hipmod.SHADOW_EXACT], images[hipmod.SHADOW_SEGMENT]
    se, ss = stats[hipmod.SHADOW_EXACT], stats[hipmod.SHADOW_SEGMENT]
    differ = int((ex.view(np.uint32) != sg.view(np.uint32)).sum())
    worst = worst_pixel_rel_l2(sg, ref)
    print(f"{scene} records={records} lens={lens_name} nee={nee} | {differ} of {ex.size} | {worst:.3e} | {ss['shadow_rays']} ({ss['shadow_rays_elided']})")
    assert np.array_equal(ex.view(np.uint32), ref.view(np.uint32))         # back in EXACT: the restatement's image, rng and counters word for word
    assert np.array_equal(rng_after.reshape(-1), np.asarray(ref_rng).reshape(-1))
    assert (se["extension_rays"], se["shadow_rays"], se["sky_evals"], se["shadow_rays_elided"]) == (st.extension_rays, st.shadow_rays, st.sky_evals, st.shadow_rays_zero_term)
    assert (scene == "open") == (st.shadow_rays == 0)                      # (the open scene has no emitter: no light is ever sampled)
    assert (ss["shadow_rays"], ss["shadow_rays_elided"], ss["extension_rays"]) == (se["shadow_rays"], se["shadow_rays_elided"], se["extension_rays"])
    assert worst < L2_BOUND, worst


# ---- plumbing

def test_default_switching_and_invalid_modes(hipmod, oracle, rpt, world):
    w = world("DarkCornell")
    W, H, spp = 160, 120, 6
    cfg = rpt.default_config(W, H, nee=1)
    seeds = rpt.blue_noise_seeds(W, H)
    ref, _, so = oracle.trace_cpu(cfg, oracle.scene(w), seeds, spp)
    r = hipmod.Renderer(0)
    try:
        assert r.shadow_mode() == hipmod.SHADOW_EXACT                  # before a scene, a configuration, anything
        r.upload_scene(w); r.set_config(cfg); r.reset(seeds)
        assert r.shadow_mode() == hipmod.SHADOW_EXACT
        for bad in (2, 3, 0xffffffff):
            with pytest.raises(hipmod.RptError) as e:
                r.set_shadow_mode(bad)
            assert e.value.code == -1 and r.shadow_mode() == hipmod.SHADOW_EXACT
        r.set_shadow_mode(hipmod.SHADOW_SEGMENT)
        with pytest.raises(hipmod.RptError):
            r.set_shadow_mode(7)
        assert r.shadow_mode() == hipmod.SHADOW_SEGMENT                # an invalid mode leaves the context as it was
        r.render(spp)
        seg, _ = r.read_accum()
        seg = seg.copy()
        assert worst_pixel_rel_l2(seg, ref) < L2_BOUND
        r.set_shadow_mode(hipmod.SHADOW_EXACT)
        r.reset(seeds)
        r.render(spp)
        again, _ = r.read_accum()
        st = r.stats()
        assert np.array_equal(again.view(np.uint32), ref.view(np.uint32))          # SEGMENT left nothing behind: the oracle's image bit for bit
        assert (st["extension_rays"], st["shadow_rays"]) == (so.extension_rays, so.shadow_rays)
    finally:
        r.close()


def test_a_switch_between_asynchronous_batches(hipmod, oracle, rpt, world):
    """Set between two rpt_render_async calls, without a wait, the mode needs no reset, disturbs no batch in flight and keeps the accumulator: 12 samples, the
    reference's ray counts, the image within the contract.  That the middle batch really ran the `_seg` kernel this test CANNOT show — both modes give the same
    accumulator words on this scene; which kernel a launch ran is visible only in a kernel trace (profiles/r10_shadow_segment_kernel_stats.csv has both names)."""
    w = world("DarkCornell")
    W, H = 200, 136
    cfg = rpt.default_config(W, H, nee=1)
    seeds = rpt.blue_noise_seeds(W, H)
    ref, _, so = oracle.trace_cpu(cfg, oracle.scene(w), seeds, 12)
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w); r.set_config(cfg); r.reset(seeds)
        r.render_async(4)
        r.set_shadow_mode(hipmod.SHADOW_SEGMENT)
        r.render_async(4)
        r.set_shadow_mode(hipmod.SHADOW_EXACT)
        r.render_async(4)
        assert r.shadow_mode() == hipmod.SHADOW_EXACT
        r.wait()
        img, s = r.read_accum()
        st = r.stats()
    finally:
        r.close()
    assert s == 12 and np.all(img[..., 3] == 12)
    assert (st["extension_rays"], st["shadow_rays"]) == (so.extension_rays, so.shadow_rays)
    print("words that differ from the oracle's image:", int((img.view(np.uint32) != ref.view(np.uint32)).sum()))
    assert worst_pixel_rel_l2(img, ref) < L2_BOUND


@pytest.mark.parametrize("ranks", [3])
def test_the_multi_driver_sets_every_rank(hipmod, rpt, world, ranks):
    w = world("DarkCornell")
    W, H = 200, 136
    cfg = rpt.default_config(W, H, nee=1)
    seeds = rpt.blue_noise_seeds(W, H)
    one = hipmod.Renderer(0)
    try:
        one.upload_scene(w); one.set_config(cfg); one.set_shadow_mode(hipmod.SHADOW_SEGMENT); one.reset(seeds)
        one.render(6)
        ref, _ = one.read_accum()
        ref = ref.copy()
        st_ref = one.stats()
    finally:
        one.close()
    m = hipmod.MultiRenderer([0] * ranks, allow_shared_device=True)
    try:
        m.upload_scene(w); m.set_config(cfg)
        with pytest.raises(hipmod.RptError) as e:
            m.set_shadow_mode(5)
        assert e.value.code == -1
        for rank in range(ranks):
            assert m.rank_view(rank).shadow_mode() == hipmod.SHADOW_EXACT
        m.set_shadow_mode(hipmod.SHADOW_SEGMENT)
        for rank in range(ranks):
            assert m.rank_view(rank).shadow_mode() == hipmod.SHADOW_SEGMENT
        m.reset(seeds)
        m.render(6)
        img, s = m.read_accum()
        st = m.stats()
    finally:
        m.close()
    assert s == 6
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert (st["extension_rays"], st["shadow_rays"], st["shadow_rays_elided"]) == (st_ref["extension_rays"], st_ref["shadow_rays"], st_ref["shadow_rays_elided"])


@pytest.mark.parametrize("scene,W,H", [("DarkCornell", 160, 120), ("VeachMIS", 160, 96)])
def test_without_nee_the_mode_changes_nothing(hipmod, rpt, world, scene, W, H):
    cfg = rpt.default_config(W, H, nee=0)
    seeds = rpt.blue_noise_seeds(W, H)
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(world(scene)); r.set_config(cfg)
        out = []
        for mode in (hipmod.SHADOW_EXACT, hipmod.SHADOW_SEGMENT):
            r.set_shadow_mode(mode)
            r.reset(seeds)
            r.render(5)
            out.append(r.read_accum()[0].copy())
            assert r.stats()["shadow_rays"] == 0
    finally:
        r.close()
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
