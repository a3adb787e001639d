"""GPU tests of the two ends of a batch on scenes whose traversal image lives in LDS, with several slots per pixel:

  * the FIRST walk of a render call starts the call's paths itself (k_traverse_nearest_stream FIRST, k_path.h begin_first_path): the call opens with
    a one-workgroup launch that zeroes its counters, no pass over the slots writes camera rays;
  * the LAST walk of a known-length batch without NEE ends its paths itself (emission of a front-facing emitter, HIT_DONE, misses into the sky queue):
    no shade launch follows it.

Every image is compared with the CPU oracle bit for bit and every ray count with the oracle's.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W0, H0 = 100, 70            # 7 000 pixels: not a multiple of 64, the last chunk of 64 pixels has padding slots


def _render(hipmod, w, cfg, seeds, batches):
    """asynchronous batches of the given sample counts, one wait: accumulators, statistics, and the statistics around the LAST batch"""
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w)
        last_walk = r.last_bounce_order()["mode"] != 0
        r.set_config(cfg); r.reset(seeds)
        for n in batches[:-1]:
            r.render_async(n)
        r.wait()
        st0 = r.stats()
        r.render_async(batches[-1])
        r.wait()
        acc, s = r.read_accum()
        st = r.stats()
    finally:
        r.close()
    assert s == sum(batches)
    return acc.copy(), st, st0, last_walk


def _same_as_oracle(oracle, cfg, w, seeds, spp, acc, st):
    acc_c, _, st_c = oracle.trace_cpu(cfg, oracle.scene(w), seeds, spp)
    assert st["extension_rays"] == st_c.extension_rays and st["sky_evals"] == st_c.sky_evals and st["shadow_rays"] == st_c.shadow_rays
    assert np.array_equal(acc.view(np.uint32), acc_c.view(np.uint32))
    return st_c


def _quad(verts, norms, tris, p, n, mat):
    k = len(verts)
    verts += [list(map(float, q)) for q in p]
    norms += [list(map(float, n))] * 4
    tris += [[k, k + 1, k + 2, mat], [k, k + 2, k + 3, mat]]


def _materials(rpt, emission):
    m = np.zeros(4, rpt._ffi.MATERIAL_DTYPE)
    m["albedo"][:] = [[0.8, 0.8, 0.8, 1], [0.7, 0.3, 0.2, 1], [0.3, 0.5, 0.8, 1], [0, 0, 0, 1]]
    m["roughness"][:, :] = np.array([0.9, 0.5, 1.0, 1.0], np.float32)[:, None]
    m["metallic"][:, :] = np.array([0.0, 0.3, 0.0, 0.0], np.float32)[:, None]
    m["emissive"][3] = emission
    return m


def tray_scene(rpt):
    """An open scene of 46 triangles: a floor of 4 x 4 quads with a low rim, two slanted panels and a small light above it.  Rays bounce in it a few
    times and leave."""
    v, n, t = [], [], []
    for i in range(4):
        for j in range(4):
            x0, z0 = -2.0 + i, -2.0 + j
            _quad(v, n, t, [(x0, 0, z0), (x0, 0, z0 + 1), (x0 + 1, 0, z0 + 1), (x0 + 1, 0, z0)], (0, 1, 0), (i + j) & 1)
    h = 0.25
    _quad(v, n, t, [(-2, 0, -2), (-2, h, -2), (-2, h, 2), (-2, 0, 2)], (1, 0, 0), 2)
    _quad(v, n, t, [(2, 0, 2), (2, h, 2), (2, h, -2), (2, 0, -2)], (-1, 0, 0), 2)
    _quad(v, n, t, [(-2, 0, 2), (-2, h, 2), (2, h, 2), (2, 0, 2)], (0, 0, -1), 2)
    _quad(v, n, t, [(2, 0, -2), (2, h, -2), (-2, h, -2), (-2, 0, -2)], (0, 0, 1), 2)
    _quad(v, n, t, [(-1.5, 0.0, 0.5), (-1.5, 0.5, 0.9), (-0.3, 0.5, 0.9), (-0.3, 0.0, 0.5)], (0, 0.6, -0.8), 2)
    _quad(v, n, t, [(0.4, 0.0, -0.2), (0.4, 0.4, -0.6), (1.6, 0.4, -0.6), (1.6, 0.0, -0.2)], (0, 0.7, 0.7), 0)
    _quad(v, n, t, [(-0.3, 1.6, -0.3), (0.3, 1.6, -0.3), (0.3, 1.6, 0.3), (-0.3, 1.6, 0.3)], (0, -1, 0), 3)
    return rpt.World.from_buffers(np.array(v, np.float32), np.array(n, np.float32), None, np.array(t, np.uint32), _materials(rpt, [12.0, 11.0, 9.0, 1.0]))


TRAY_VIEW = dict(cam_position=(0.0, 2.2, -3.6, 0.0), cam_rotation=(0.55, 0.0, 0.0, 0.0))


def lamp_box_scene(rpt, flip=False):
    """A closed box with ONE emissive triangle floating in it: its front faces the floor, its back the ceiling (flip: the other way round — the same
    plane, the same paths up to the ray that hits it, front and back exchanged)."""
    v, n, t = [], [], []
    c = [(-2, 0, -2), (2, 0, -2), (2, 0, 2), (-2, 0, 2), (-2, 3, -2), (2, 3, -2), (2, 3, 2), (-2, 3, 2)]
    for q, nrm, mat in [((0, 3, 2, 1), (0, 1, 0), 0), ((4, 5, 6, 7), (0, -1, 0), 0), ((3, 7, 6, 2), (0, 0, -1), 1), ((0, 1, 5, 4), (0, 0, 1), 1),
                        ((0, 4, 7, 3), (1, 0, 0), 2), ((1, 2, 6, 5), (-1, 0, 0), 2)]:
        _quad(v, n, t, [c[i] for i in q], nrm, mat)
    k = len(v)
    v += [[-1.4, 1.5, -1.2], [1.4, 1.5, -1.2], [0.0, 1.5, 1.5]]
    n += [[0, -1, 0]] * 3
    t += [[k, k + 2, k + 1, 3] if flip else [k, k + 1, k + 2, 3]]
    return rpt.World.from_buffers(np.array(v, np.float32), np.array(n, np.float32), None, np.array(t, np.uint32), _materials(rpt, [6.0, 5.0, 4.0, 1.0]))


LAMP_VIEW = dict(cam_position=(0.0, 1.0, -1.9, 0.0))


def _last_ray_counts(oracle, rpt, w, seeds, W, H, spp, view):
    """from the oracle alone: the rays of the last bounce (max_bounces 4, no roulette before it) and how many of them miss — the difference of the
    counts of a 4-bounce and a 3-bounce render, whose paths agree up to there"""
    st = {}
    for mb in (3, 4):
        cfg = rpt.default_config(W, H, nee=0, min_bounces=3, max_bounces=mb, **view)
        st[mb] = oracle.trace_cpu(cfg, oracle.scene(w), seeds, spp)[2]
    return st[4].extension_rays - st[3].extension_rays, st[4].sky_evals - st[3].sky_evals


def _last_rays_adding_emission(oracle, rpt, w, seeds, W, H, view):
    """from the oracle alone, one sample per pixel: the pixels whose LAST ray adds something when the sky adds nothing (sun intensity 0) — the
    rays that end on the FRONT of an emitter at bounce max_bounces - 1"""
    acc = {}
    for mb in (3, 4):
        cfg = rpt.default_config(W, H, nee=0, min_bounces=3, max_bounces=mb, **view)
        cfg.sun_direction[3] = 0.0
        acc[mb] = oracle.trace_cpu(cfg, oracle.scene(w), seeds, 1)[0]
    return int(np.any(acc[3][..., :3] != acc[4][..., :3], axis=2).sum())


@pytest.mark.parametrize("q_shift", [None, "3"])
@pytest.mark.parametrize("scene", ["DarkCornell", "FurnaceTest"])
def test_known_length_batches_of_changing_length(monkeypatch, hipmod, oracle, rpt, world, scene, q_shift):
    """Asynchronous batches of 5, 8, 3, 16 and 6 samples at 100 x 70: padding slots behind the last pixel, batches shorter than their slots per pixel
    (5 of 8, 3 of 4, 6 of 8: the slots with k >= n_samples stay idle and serve the next, longer batch), in both slot layouts."""
    monkeypatch.delenv("RPT_LAST_ORDER", raising=False)
    if q_shift is None:
        monkeypatch.delenv("RPT_SLOT_Q_SHIFT", raising=False)
    else:
        monkeypatch.setenv("RPT_SLOT_Q_SHIFT", q_shift)
    w = world(scene)
    cfg = rpt.default_config(W0, H0, nee=0)
    seeds = rpt.blue_noise_seeds(W0, H0)
    batches = (5, 8, 3, 16, 6)
    acc, st, _, last_walk = _render(hipmod, w, cfg, seeds, batches)
    assert last_walk == (scene == "DarkCornell")              # FurnaceTest (10 240 triangles, half of them emissive) is walked from global memory: every launch as before
    _same_as_oracle(oracle, cfg, w, seeds, sum(batches), acc, st)


@pytest.mark.parametrize("scene,nee,last_order,shade_launches", [("DarkCornell", 0, None, 3), ("FurnaceTest", 0, None, 4), ("DarkCornell", 0, "off", 4),
                                                                  ("DarkCornell", 1, None, 4), ("VeachMIS", 0, None, 4)])
def test_launches_of_a_known_length_batch(monkeypatch, hipmod, oracle, rpt, world, scene, nee, last_order, shade_launches):
    """rpt_stats.kernel_launches around one batch with max_bounces = 4: four traversal launches; three shade launches where the last walk ends the
    paths (an LDS scene, no NEE), four with RPT_LAST_ORDER=off, with NEE and on the scenes walked from global memory (FurnaceTest, VeachMIS).  One generate launch (the stage
    that opens the call) and one completion either way."""
    monkeypatch.delenv("RPT_LAST_ORDER", raising=False)
    monkeypatch.delenv("RPT_SLOT_Q_SHIFT", raising=False)
    if last_order is not None:
        monkeypatch.setenv("RPT_LAST_ORDER", last_order)
    w = world(scene)
    cfg = rpt.default_config(W0, H0, nee=nee, min_bounces=3, max_bounces=4)
    seeds = rpt.blue_noise_seeds(W0, H0)
    acc, st, st0, last_walk = _render(hipmod, w, cfg, seeds, (8, 8))
    assert last_walk == (scene == "DarkCornell" and last_order is None)      # (the last walk ends paths: DarkCornell only; FurnaceTest and VeachMIS do not live in LDS)
    d = {k: st["kernel_launches"][k] - st0["kernel_launches"][k] for k in st["kernel_launches"]}
    print("launches of the batch:", d)
    assert d["traverse"] == 4 and d["shade"] == shade_launches and d["generate"] == 1 and d["complete"] == 1 and d["sky"] == 1
    assert d["shadow"] == (4 if nee else 0)
    _same_as_oracle(oracle, cfg, w, seeds, 16, acc, st)


@pytest.mark.parametrize("compact", [None, "1"])
def test_last_rays_that_miss_in_bulk(monkeypatch, hipmod, oracle, rpt, compact):
    """An open scene in LDS (tray_scene) at 200 x 140, 32 samples in one batch: more than half of the rays of the last bounce leave the scene, so the
    walk's own sky-queue reservations run at queue-filling rates — with the shade stage in either variant (the shard a slot is reserved in follows it)."""
    monkeypatch.delenv("RPT_LAST_ORDER", raising=False)
    monkeypatch.delenv("RPT_SLOT_Q_SHIFT", raising=False)
    if compact is None:
        monkeypatch.delenv("RPT_SHADE_COMPACT", raising=False)
    else:
        monkeypatch.setenv("RPT_SHADE_COMPACT", compact)
    W, H, spp = 200, 140, 32
    w = tray_scene(rpt)
    seeds = rpt.blue_noise_seeds(W, H)
    last, missing = _last_ray_counts(oracle, rpt, w, seeds, W, H, spp, TRAY_VIEW)
    print(f"tray scene: {len(w.indices)} triangles; {last} rays at the last bounce, {missing} of them miss ({missing / last:.3f})")
    assert last > 20000 and missing > 0.5 * last        # the scene is fit for the purpose
    cfg = rpt.default_config(W, H, nee=0, min_bounces=3, max_bounces=4, **TRAY_VIEW)
    acc, st, st0, last_walk = _render(hipmod, w, cfg, seeds, (spp, spp))
    assert last_walk and st["kernel_launches"]["shade"] - st0["kernel_launches"]["shade"] == 3
    _same_as_oracle(oracle, cfg, w, seeds, 2 * spp, acc, st)


def test_an_emitter_at_the_last_bounce_front_and_back(monkeypatch, hipmod, oracle, rpt):
    """A two-sided case (lamp_box_scene): last rays that end on the emissive triangle's front — its emission is added, throughput times emission, masked
    when not finite — and last rays that end on its back, which add nothing.  Both in the scene as built and with the triangle's winding reversed."""
    monkeypatch.delenv("RPT_LAST_ORDER", raising=False)
    monkeypatch.delenv("RPT_SLOT_Q_SHIFT", raising=False)
    seeds = rpt.blue_noise_seeds(W0, H0)
    front = _last_rays_adding_emission(oracle, rpt, lamp_box_scene(rpt, False), seeds, W0, H0, LAMP_VIEW)
    back = _last_rays_adding_emission(oracle, rpt, lamp_box_scene(rpt, True), seeds, W0, H0, LAMP_VIEW)     # (the flipped scene's fronts)
    print(f"lamp box, one sample per pixel: {front} last rays end on the emitter's front, {back} on its back")
    assert front > 50 and back > 50
    for flip in (False, True):
        w = lamp_box_scene(rpt, flip)
        cfg = rpt.default_config(W0, H0, nee=0, min_bounces=3, max_bounces=4, **LAMP_VIEW)
        acc, st, st0, last_walk = _render(hipmod, w, cfg, seeds, (8, 8))
        assert last_walk and st["kernel_launches"]["shade"] - st0["kernel_launches"]["shade"] == 3
        _same_as_oracle(oracle, cfg, w, seeds, 16, acc, st)


@pytest.mark.parametrize("batches", [1, 2])
def test_a_short_batch_is_noticed_where_the_first_walk_starts_the_paths(hipmod, rpt, world, batches):
    """rpt_debug_short_batch at 640 x 360 x 8 slots (1.8 M slots: every persistent workgroup of the walk takes spans): the last batch is caught by
    rpt_wait, an earlier one by the walk that takes its slots for the next batch."""
    w = world("DarkCornell")
    W, H = 640, 360
    cfg = rpt.default_config(W, H)
    seeds = rpt.blue_noise_seeds(W, H)
    r = hipmod.Renderer(0)
    try:
        r.debug_short_batch(True)
        r.upload_scene(w); r.set_config(cfg); r.reset(seeds)
        for _ in range(batches):
            r.render_async(8)
        with pytest.raises(hipmod.RptError, match="in flight"):
            r.wait()
    finally:
        r.close()
    r = hipmod.Renderer(0)
    try:
        r.upload_scene(w); r.set_config(cfg); r.reset(seeds)
        for _ in range(3):
            r.render_async(8)
        r.wait()                                        # complete batches pass
        assert r.read_accum()[1] == 24
    finally:
        r.close()
