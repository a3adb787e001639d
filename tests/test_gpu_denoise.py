"""The denoiser on the device (rpt_denoise, rpt_read_guides, rpt_multi_denoise; csrc/k_denoise.h): the guide buffers against the numpy restatement over the
oracle's hits, the filter against the host build of the same header bit for bit, no side effects on the render state, independence of the GPU count,
the error cases, and the host mirror's denoise switch."""
import numpy as np
import pytest

import denoise_ref
from scenes import textured_scene

pytestmark = pytest.mark.gpu

TEXTURED_CAMERA = {"cam_position": (0.0, 1.6, -4.0, 0.0), "cam_rotation": (0.05, 0.1, 0.0, 0.0)}


def load(world, scene):
    return textured_scene()[0] if scene == "textured" else world(scene)


def config(rpt, scene, w, h, nee=0, **over):
    if scene == "textured":
        over = {**TEXTURED_CAMERA, **over}
    return rpt.default_config(w, h, nee=nee, **over)


def begin(renderer, rpt, wld, cfg, spp):
    renderer.upload_scene(wld)
    renderer.set_config(cfg)
    renderer.reset(rpt.blue_noise_seeds(cfg.width, cfg.height))
    if spp:
        renderer.render(spp)


def same_bits(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def host_denoise(hipmod, renderer, params=None, op=0):
    """denoise_host fed the device's own guides and accumulator"""
    acc, n = renderer.read_accum()
    g = renderer.guides()
    mean = (acc[..., :3] / np.float32(n)).astype(np.float32)
    return hipmod.denoise_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], params, op)


@pytest.mark.parametrize("scene,w,h,kinds", [("DarkCornell", 128, 128, 2), ("VeachMIS", 160, 90, 2), ("PBRTest", 96, 64, 2), ("FurnaceTest", 64, 64, 2), ("textured", 128, 96, 2),
                                             ("DarkCornell", 70, 9, 1), ("VeachMIS", 70, 9, 2), ("DarkCornell", 1, 1, 1)])
def test_guides_match_the_numpy_restatement(renderer, rpt, world, oracle, scene, w, h, kinds):
    """kind equal; depth bitwise the oracle's t; untextured albedo bitwise; normals, positions and textured albedo within 1e-6 absolute (a handful of f32
    roundings on values of order one; a miss's position, ro + rd * 1e6, is the same three operations on both sides and is compared bitwise)"""
    wld, cfg = load(world, scene), config(rpt, scene, w, h)
    begin(renderer, rpt, wld, cfg, 0)
    got, want = renderer.guides(), denoise_ref.guides(wld, cfg, oracle)
    assert np.array_equal(got["kind"], want["kind"])
    assert len(np.unique(want["kind"])) >= kinds                                         # (the case covers what it is there for: the 70x9 strip of the closed box sees walls only)
    assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32))
    miss = want["kind"] == 0
    assert np.all(got["depth"][miss] == np.float32(1e6)) and np.all(got["normal"][miss] == 0) and np.all(got["albedo"][want["kind"] != 1] == 1)
    assert np.array_equal(got["position"][miss].view(np.uint32), want["position"][miss].view(np.uint32))
    if getattr(wld, "atlas", None) is None:
        assert np.array_equal(got["albedo"].view(np.uint32), want["albedo"].view(np.uint32))
    else:
        err = np.abs(got["albedo"] - want["albedo"]).max()
        print(f"{scene}: textured albedo max abs difference {err:.3e}")
        assert err <= 1e-6
        assert np.unique(got["albedo"][want["kind"] == 1], axis=0).shape[0] > 50        # (the texture is there)
    e_n, e_p = np.abs(got["normal"] - want["normal"]).max(), np.abs(got["position"][~miss] - want["position"][~miss]).max() if (~miss).any() else 0.0
    print(f"{scene} {w}x{h}: normals max abs difference {e_n:.3e}, positions {e_p:.3e}")
    assert e_n <= 1e-6 and e_p <= 1e-6
    length = np.linalg.norm(got["normal"].astype(np.float64), axis=-1)
    assert np.all((np.abs(length - 1) < 1e-6) | (length == 0))


@pytest.mark.parametrize("scene,w,h,nee", [("DarkCornell", 256, 256, 0), ("VeachMIS", 320, 180, 1), ("textured", 128, 96, 1), ("DarkCornell", 70, 9, 0), ("DarkCornell", 1, 1, 0)])
def test_device_filter_equals_the_host_build_bitwise(renderer, rpt, hipmod, world, scene, w, h, nee):
    wld, cfg = load(world, scene), config(rpt, scene, w, h, nee)
    begin(renderer, rpt, wld, cfg, 8)
    for op in range(7):
        assert same_bits(renderer.denoise(tonemap_op=op), host_denoise(hipmod, renderer, None, op)), f"defaults, op {op}"
    for it, dem, sc in [(0, 1, 2.0), (1, 0, 0.0), (6, 1, 0.7), (5, 0, 4.0)]:
        p = hipmod.denoise_params(iterations=it, demodulate=dem, sigma_color=sc)
        assert same_bits(renderer.denoise(params=p, tonemap_op=it % 7), host_denoise(hipmod, renderer, p, it % 7)), f"iterations {it} demodulate {dem} sigma_color {sc}"
    assert same_bits(renderer.denoise(params=hipmod.denoise_params(iterations=0), tonemap_op=2), renderer.resolve(2))
    if w * h > 1000:
        assert not same_bits(renderer.denoise(), renderer.resolve(0))                   # (it does filter)


def test_denoise_has_no_side_effects_and_caches_its_guides(renderer, rpt, hipmod, world):
    """render 8, denoise, render 8 more == 16 rendered without the call: accumulator, rng and counters bit-identical; guides rebuilt on the first call, cached
    on the second, rebuilt after a set_config that moves the camera (and after a new scene)"""
    w = h = 128
    wld, cfg = world("DarkCornell"), rpt.default_config(w, h, nee=1)
    begin(renderer, rpt, wld, cfg, 8)
    renderer.render(8)
    acc_ref, n_ref = renderer.read_accum()
    rng_ref, stats_ref = renderer.read_rng(), renderer.stats()
    begin(renderer, rpt, wld, cfg, 8)
    mode = renderer.shadow_mode()
    first, rep1 = renderer.denoise(with_report=True)
    again, rep2 = renderer.denoise(with_report=True)
    assert rep1["guides_rebuilt"] == 1 and rep1["guides_ms"] > 0 and rep1["device_ms"] > 0
    assert rep2["guides_rebuilt"] == 0 and rep2["guides_ms"] == 0 and rep2["device_ms"] > 0 and same_bits(first, again)
    assert renderer.shadow_mode() == mode
    renderer.render(8)
    acc, n = renderer.read_accum()
    assert n == n_ref == 16 and same_bits(acc, acc_ref) and np.array_equal(renderer.read_rng(), rng_ref)
    stats = renderer.stats()
    for k in ("samples", "extension_rays", "shadow_rays", "shadow_rays_elided", "sky_evals", "light_index_clamped"):
        assert stats[k] == stats_ref[k], k
    moved = rpt.default_config(w, h, nee=1, cam_position=(0.3, 1.2, -5.0, 0.0))
    g_before = renderer.guides()
    renderer.set_config(moved)                                                          # same size: the accumulator stays, the guides do not
    out, rep3 = renderer.denoise(with_report=True)
    assert rep3["guides_rebuilt"] == 1 and not np.array_equal(renderer.guides()["depth"], g_before["depth"])
    assert renderer.denoise(with_report=True)[1]["guides_rebuilt"] == 0
    renderer.upload_scene(world("VeachMIS"))
    assert renderer.denoise(with_report=True)[1]["guides_rebuilt"] == 1
    renderer.set_config(rpt.default_config(96, 64))                                     # a resize releases the buffers; the next use sizes them anew
    renderer.reset(rpt.blue_noise_seeds(96, 64))
    renderer.render(2)
    out, rep = renderer.denoise(with_report=True)
    assert out.shape == (64, 96, 3) and rep["guides_rebuilt"] == 1 and same_bits(out, host_denoise(hipmod, renderer))


def test_denoise_between_asynchronous_batches(renderer, rpt, hipmod, world):
    w = h = 96
    wld, cfg = world("DarkCornell"), rpt.default_config(w, h)
    begin(renderer, rpt, wld, cfg, 0)
    renderer.render_async(8)
    out = renderer.denoise()                                                            # synchronises by itself
    assert same_bits(out, host_denoise(hipmod, renderer))
    renderer.render_async(8)
    renderer.wait()
    assert renderer.read_accum()[1] == 16


def test_denoise_does_not_depend_on_the_gpu_count(renderer, rpt, hipmod, world):
    """three ranks on one device, gathered == one context; GATHERED after comm_init_local == ACCUM"""
    w, h = 200, 130
    wld, cfg, seeds = world("DarkCornell"), rpt.default_config(w, h, nee=1), rpt.blue_noise_seeds(w, h)
    begin(renderer, rpt, wld, cfg, 8)
    one = renderer.denoise(tonemap_op=3)
    m = hipmod.MultiRenderer([0, 0, 0], allow_shared_device=True)
    try:
        m.upload_scene(wld)
        m.set_config(cfg)
        m.reset(seeds)
        m.render(8)
        many, rep = m.denoise(tonemap_op=3, with_report=True)
        assert rep["guides_rebuilt"] == 1 and same_bits(many, one)
        assert m.denoise(tonemap_op=3, with_report=True)[1]["guides_rebuilt"] == 0
        with pytest.raises(hipmod.RptError) as e:                                       # a rank of several has no whole accumulator
            m.rank_view(1).denoise()
        assert e.value.code == -1
        with pytest.raises(hipmod.RptError) as e:                                       # ... and no gathered image
            m.rank_view(1).denoise(source=hipmod.DENOISE_GATHERED)
        assert e.value.code == -1
        m.render(8)                                                                     # still usable
        assert m.read_accum()[1] == 16
    finally:
        m.close()
    r = hipmod.Renderer(0)
    try:
        begin(r, rpt, wld, cfg, 0)
        r.comm_init_local()
        with pytest.raises(hipmod.RptError) as e:                                       # before any gather
            r.denoise(source=hipmod.DENOISE_GATHERED)
        assert e.value.code == -1
        r.render_async(8)
        r.gather_async()
        r.render_async(8)                                                               # the next batch renders while batch 1 is denoised
        assert same_bits(r.denoise(source=hipmod.DENOISE_GATHERED, tonemap_op=3), one)  # the gather's sample count (8), not the context's
        r.wait()
        assert r.read_accum()[1] == 16
    finally:
        r.close()


def test_every_refusal_leaves_the_context_usable(renderer, rpt, hipmod, world):
    w = h = 64
    begin(renderer, rpt, world("DarkCornell"), rpt.default_config(w, h), 0)
    with pytest.raises(hipmod.RptError) as e:                                           # zero samples
        renderer.denoise()
    assert e.value.code == -1 and "zero samples" in str(e.value)
    renderer.render(4)
    good = renderer.denoise()
    bad = [dict(params=hipmod.denoise_params(iterations=7)), dict(params=hipmod.denoise_params(normal_power_log2=11)), dict(params=hipmod.denoise_params(sigma_color=-0.5)),
           dict(params=hipmod.denoise_params(sigma_plane=float("inf"))), dict(params=hipmod.denoise_params(sigma_color=float("nan"))), dict(tonemap_op=7), dict(source=2)]
    for kw in bad:
        with pytest.raises(hipmod.RptError) as e:
            renderer.denoise(**kw)
        assert e.value.code == -1, kw
        assert same_bits(renderer.denoise(), good), kw
    renderer.render(4)
    assert renderer.read_accum()[1] == 8


@pytest.mark.parametrize("overlap", [True, False])
def test_host_mirror_publishes_the_denoised_image(renderer, rpt, hipmod, world, overlap):
    """rpt_trace_gpu with state.denoise on publishes what Renderer.denoise gives for the same state; with `interacting` raised (every iteration flushes) the
    plain mean, as the reference's `&& !flush` (trace.rs:208)"""
    w = h = 96
    state = rpt.setup_trace(w, h, 16)
    state.set_sync_rate(8)
    state.set_overlap(overlap)
    state.set_denoise(True)
    rpt.trace_gpu(rpt.fixture("DarkCornell.glb"), None, state)
    assert state.samples == 16
    fb = np.array(state.framebuffer(), np.float32).reshape(h, w, 3)
    begin(renderer, rpt, world("DarkCornell"), rpt.default_config(w, h), 8)
    renderer.render(8)
    assert same_bits(fb, renderer.denoise()) and not same_bits(fb, renderer.resolve(0))
    state.close()
    begin(renderer, rpt, world("DarkCornell"), rpt.default_config(w, h), 1)
    plain, filtered = renderer.resolve(0), renderer.denoise()                           # a 1-sample image, unfiltered and filtered
    assert not same_bits(plain, filtered)
    state = rpt.setup_trace(w, h, 1)
    state.set_overlap(overlap)
    state.set_denoise(True)
    state.set_interacting(True)
    import threading
    import time
    t = threading.Thread(target=lambda: rpt.trace_gpu(rpt.fixture("DarkCornell.glb"), None, state))
    t.start()
    deadline, seen = time.time() + 120, []
    while time.time() < deadline and t.is_alive() and len(seen) < 3:                    # three looks at what the drag publishes
        fb = np.array(state.framebuffer(), np.float32).reshape(h, w, 3)
        if fb.any():
            seen.append(fb)
        time.sleep(0.001)
    state.set_running(False)
    t.join(120)
    assert not t.is_alive() and len(seen) == 3
    assert all(same_bits(fb, plain) for fb in seen)
    state.close()
