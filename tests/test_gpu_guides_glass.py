"""Guides that follow glass on the device (rpt_set_guides_through_glass, rpt_guides_info_get; csrc/k_guides_glass.h) against the CPU chain — the numpy
restatement of tests/guides_glass_ref.py over the oracle's walk, which tests/test_guides_glass.py holds the host build of the step to — bit for bit: every
plane of rpt_read_guides and the counts; the setting off and all-PBR records against the first-hit guides byte for byte; what rebuilds the guides; a view
without glass; the three denoisers against their host builds fed the CPU chain's guides; three ranks on one device; re-upload, resize, destroy; and the
chain under a camera lens (rpt_set_camera_lens), which starts from the rays through the lens centre (csrc/rpt_lens.hip k_dn_camera_rays_lens feeding
build_guides_through_glass): the CPU chain over tests/lens_ref.py centre_rays."""
import numpy as np
import pytest

import guides_glass_ref as ref
import lens_ref
import model_scenes

pytestmark = pytest.mark.gpu

F = np.float32
W, H, SPP = 80, 72, 8
PLANES = ("albedo", "normal", "depth", "position", "kind")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return a.shape == b.shape and np.array_equal(a, b)


def same_image(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.fixture(scope="module")
def r(hipmod):
    """a Renderer of the module's own: it carries the setting and moments, which the session's renderer must not"""
    r = hipmod.Renderer(0)
    yield r
    r.close()


def config(name, w=W, h=H, **view):
    """the scene's configuration without NEE, the camera fields of `view` replaced"""
    cfg = model_scenes.config(name, 0, w, h)
    for k, v in view.items():
        getattr(cfg, k)[:] = v
    return cfg


_cpu = {}


def cpu_chain(oracle, name, K, w=W, h=H, **view):
    """the restatement's guides and counts, computed once per process"""
    key = (name, K, w, h, tuple(sorted(view.items())))
    if key not in _cpu:
        world, rec, skybox, _ = model_scenes.scene(name)
        cfg = config(name, w, h, **view)
        _cpu[key] = ref.guides(world, rec, K, cfg, oracle, oracle.scene(world, skybox_f32=skybox))
    return _cpu[key]


def prepare(r, rpt, name, K, w=W, h=H, records=True, spp=0, **view):
    world, rec, skybox, _ = model_scenes.scene(name)
    r.upload_scene(world, skybox_f32=skybox)
    if records:
        r.set_material_models(rec)
    r.set_guides_through_glass(K)
    r.set_config(config(name, w, h, **view))
    r.reset(rpt.blue_noise_seeds(w, h))
    if spp:
        r.render(spp)
    return world, rec


def check_guides(got, want, what):
    for k in PLANES:
        assert same_bits(got[k], want[k]), f"{what}: {k} differs in {np.count_nonzero(got[k] != want[k])} entries"


def check_info(info, want, K):
    assert info["max_interfaces"] == K
    for k in ("rounds", "rays", "pixels_through_glass", "pixels_exhausted"):
        assert info[k] == want[k], (k, info, want)


@pytest.mark.parametrize("name,K,w,h", [(n, K, W, H) for n in ("room", "open", "textured") for K in (1, 2, 8)] + [("room", 4, 37, 23)])
def test_guides_and_counts_equal_the_cpu_chain(r, rpt, oracle, name, K, w, h):
    prepare(r, rpt, name, K, w, h)
    want, want_info = cpu_chain(oracle, name, K, w, h)
    check_guides(r.guides(), want, f"{name} K={K} {w}x{h}")
    check_info(r.guides_info(), want_info, K)
    assert want_info["pixels_through_glass"] > 0 and want_info["rounds"] >= 2


def test_setting_off_and_all_pbr_records_are_the_first_hit_guides(r, rpt, oracle):
    for name in ("room", "textured"):
        world, rec = prepare(r, rpt, name, 0)
        off = r.guides()
        info = r.guides_info()
        assert info["max_interfaces"] == 0 and info["rounds"] == 1 and info["rays"] == [W * H] + [0] * 8 and info["pixels_through_glass"] == 0
        assert r.guides_through_glass() == 0
        r.set_guides_through_glass(4)
        r.set_material_models(model_scenes.records([model_scenes.MODEL_PBR] * len(rec)))
        check_guides(r.guides(), off, name + ": K = 4, every record PBR")
        assert r.guides_info()["rounds"] == 1 and r.guides_through_glass() == 4
        r.set_material_models(None)
        check_guides(r.guides(), off, name + ": K = 4, no records")
        # with the records back, the chain kernel's records of a pixel whose chain met no glass are the first-hit kernel's, byte for byte
        r.set_material_models(rec)
        on = r.guides()
        want, _ = cpu_chain(oracle, name, 4)
        check_guides(on, want, name + " K=4")
        untouched = same = (on["depth"].view(np.uint32) == off["depth"].view(np.uint32)) & (on["kind"] == off["kind"])
        for k in ("albedo", "normal", "position"):
            same = same & (on[k].view(np.uint32) == off[k].view(np.uint32)).all(axis=-1)
        first_material = world.indices[oracle.trace_rays(oracle.scene(world), 0, *ref.camera_rays(model_scenes.config(name, 0, W, H), oracle))[1]]["material"].reshape(H, W)
        no_glass = (rec["model"][first_material] != model_scenes.MODEL_GLASS) | (off["kind"] != 1)
        assert no_glass.sum() > 1000 and np.all(same[no_glass]) and not np.all(untouched)


def test_what_rebuilds_the_guides(r, rpt, hipmod):
    world, rec = prepare(r, rpt, "room", 0, spp=1)
    rebuilt = lambda: r.denoise(with_report=True)[1]["guides_rebuilt"]
    assert rebuilt() == 1 and rebuilt() == 0
    r.set_material_models(rec)                                                              # K = 0: the records do not touch the guides
    assert rebuilt() == 0
    r.set_guides_through_glass(0)
    assert rebuilt() == 0
    r.set_guides_through_glass(2)
    assert rebuilt() == 1 and rebuilt() == 0
    r.set_guides_through_glass(2)                                                           # the same value: nothing is stale
    assert rebuilt() == 0
    r.set_guides_through_glass(4)
    assert rebuilt() == 1
    r.set_material_models(model_scenes.records(rec["model"], np.where(rec["model"] == 2, 1.3, 0.0)))      # K > 0: new records, new guides
    assert rebuilt() == 1 and rebuilt() == 0
    with pytest.raises(hipmod.RptError) as e:
        r.set_guides_through_glass(9)
    assert e.value.code == -1 and "0..8" in str(e.value) and r.guides_through_glass() == 4 and rebuilt() == 0
    r.set_guides_through_glass(0)
    assert rebuilt() == 1
    assert hipmod.lib().rpt_guides_through_glass(r._h, None) == -1 and hipmod.lib().rpt_guides_info_get(r._h, None) == -1
    assert hipmod.lib().rpt_set_guides_through_glass(None, 1) == -1


def test_a_view_without_glass_ends_after_the_first_round(r, rpt, oracle):
    """the open scene seen with the sphere behind the camera: a Glass record, no glass pixel"""
    view = dict(cam_rotation=(0.1, 3.14159274, 0.0, 0.0))
    prepare(r, rpt, "open", 0, **view)
    off = r.guides()
    r.set_guides_through_glass(8)
    check_guides(r.guides(), off, "open, looking away")
    info = r.guides_info()
    assert info["rounds"] == 1 and info["rays"] == [W * H] + [0] * 8 and info["pixels_through_glass"] == 0 and info["pixels_exhausted"] == 0
    want, want_info = cpu_chain(oracle, "open", 8, **view)
    check_guides(off, want, "open, looking away, against the chain")
    check_info(info, want_info, 8)


def mean_of(r):
    acc, n = r.read_accum()
    return (acc[..., :3] / F(n)).astype(F)


def test_the_three_denoisers_equal_their_host_builds_on_the_chains_guides(r, rpt, hipmod, oracle):
    """the filters did not change: this proves the wiring.  8 spp of the room, K = 4; the temporal call over two views"""
    K = 4
    world, rec, skybox, _ = model_scenes.scene("room")
    r.upload_scene(world, skybox_f32=skybox)
    r.set_material_models(rec)
    r.set_guides_through_glass(K)
    r.set_moments(True)
    r.temporal_reset()
    cam_a = model_scenes.config("room", 0, W, H)
    move = dict(cam_position=(0.2, 1.6, -0.8, 0.0), cam_rotation=(0.12, 0.05, 0.0, 0.0))
    cam_b = config("room", **move)
    planes = lambda g: (g["albedo"], g["normal"], g["position"], g["depth"], g["kind"])
    try:
        r.set_config(cam_a)
        r.reset(rpt.blue_noise_seeds(W, H))
        r.render(SPP)
        ga, _ = cpu_chain(oracle, "room", K)
        mean, moments = mean_of(r), r.read_moments()
        assert same_image(r.denoise(), hipmod.denoise_host(mean, *planes(ga)))
        p = hipmod.denoise_var_params(sigma_variance=4.0)
        rgb, var = r.denoise_variance(params=p)
        want = hipmod.denoise_variance_host(mean, *planes(ga), moments, p)
        assert same_image(rgb, want[0]) and same_image(var, want[1])
        tp = hipmod.temporal_params(sigma_variance=4.0)
        a = hipmod.denoise_temporal_host(mean, *planes(ga), moments, cam_a, None, tp, 0)
        rgb, var, hist, rep = r.denoise_temporal(params=tp, with_report=True)
        assert same_image(rgb, a["rgb"]) and same_image(var, a["variance"]) and same_image(hist, a["history"]) and rep["pixels_with_history"] == 0
        r.set_config(cam_b)
        r.reset(rpt.blue_noise_seeds(W, H))
        r.render(SPP)
        gb, _ = cpu_chain(oracle, "room", K, **move)
        previous = {"camera": cam_a.copy(), "normal": ga["normal"], "position": ga["position"], "kind": ga["kind"], "records": a["records"]}
        b = hipmod.denoise_temporal_host(mean_of(r), *planes(gb), r.read_moments(), cam_b, previous, tp, 0)
        rgb, var, hist, rep = r.denoise_temporal(params=tp, with_report=True)
        assert same_image(rgb, b["rgb"]) and same_image(var, b["variance"]) and same_image(hist, b["history"])
        assert rep["pixels_with_history"] == b["pixels_with_history"] > 0 and rep["guides_rebuilt"] == 1
    finally:
        r.set_moments(False)
        r.temporal_reset()


def test_three_ranks_on_one_device(hipmod, rpt, oracle):
    K = 4
    world, rec, skybox, _ = model_scenes.scene("room")
    want, want_info = cpu_chain(oracle, "room", K)
    m = hipmod.MultiRenderer([0, 0, 0], allow_shared_device=True)
    try:
        m.upload_scene(world, skybox_f32=skybox)
        m.set_material_models(rec)
        m.set_guides_through_glass(K)
        m.set_config(model_scenes.config("room", 0, W, H))
        m.reset(rpt.blue_noise_seeds(W, H))
        m.render(SPP)
        acc, n = m.read_accum()
        mean = (acc[..., :3] / F(n)).astype(F)
        out = m.denoise()
        assert same_image(out, hipmod.denoise_host(mean, want["albedo"], want["normal"], want["position"], want["depth"], want["kind"]))
        for k in range(3):
            view = m.rank_view(k)
            assert view.guides_through_glass() == K
        root = m.rank_view(0)
        check_guides(root.guides(), want, "rank 0 of 3")
        check_info(root.guides_info(), want_info, K)
    finally:
        m.close()


def test_reupload_resize_destroy(hipmod, rpt, oracle):
    r = hipmod.Renderer(0)
    try:
        prepare(r, rpt, "room", 4)
        check_guides(r.guides(), cpu_chain(oracle, "room", 4)[0], "room")
        world, rec, skybox, _ = model_scenes.scene("open")
        r.upload_scene(world, skybox_f32=skybox)                                            # the records are gone, the setting stays
        r.set_config(model_scenes.config("open", 0, W, H))
        r.reset(rpt.blue_noise_seeds(W, H))
        assert r.guides_through_glass() == 4
        first = r.guides()
        assert r.guides_info()["rounds"] == 1
        r.set_material_models(rec)
        check_guides(r.guides(), cpu_chain(oracle, "open", 4)[0], "open after a re-upload")
        assert r.guides_info()["rounds"] >= 2 and not same_bits(first["depth"], r.guides()["depth"])
        r.set_config(model_scenes.config("open", 0, 37, 23))                               # a resize releases the buffers; the next use sizes them anew
        r.reset(rpt.blue_noise_seeds(37, 23))
        check_guides(r.guides(), cpu_chain(oracle, "open", 4, 37, 23)[0], "open 37x23")
    finally:
        r.close()                                                                           # with the guides of a chain build alive


# ---- under a camera lens ---------------------------------------------------------------------------------------------------------------------------------
def cpu_chain_under(oracle, name, K, lens_name, w=W, h=H):
    """the chain over the lens-centre rays, computed once per process; the aperture does not enter (lens_ref.centre_rays takes the field of view alone)"""
    tan_half = lens_ref.LENSES[lens_name][0]
    key = (name, K, w, h, "tan_half", tan_half)
    if key not in _cpu:
        world, rec, skybox, _ = model_scenes.scene(name)
        cfg = config(name, w, h)
        _cpu[key] = ref.guides(world, rec, K, cfg, oracle, oracle.scene(world, skybox_f32=skybox), rays=lens_ref.centre_rays(cfg, tan_half, oracle))
    return _cpu[key]


def prepare_under(r, rpt, name, K, lens_name, w=W, h=H, spp=0):
    """prepare with the lens; the configuration without NEE and min_bounces 3: 30 dimensions, which an aperture leaves the path"""
    world, rec, skybox, _ = model_scenes.scene(name)
    r.set_camera_lens(None)
    r.upload_scene(world, skybox_f32=skybox)
    r.set_material_models(rec)
    r.set_guides_through_glass(K)
    cfg = model_scenes.config(name, 0, w, h, **model_scenes.APERTURE_OVERRIDES[0])
    r.set_config(cfg)
    r.set_camera_lens(lens_ref.lens(lens_name))
    r.reset(rpt.blue_noise_seeds(w, h))
    if spp:
        r.render(spp)
    return world, rec, cfg


@pytest.fixture
def lens_off(r):
    yield r
    r.set_camera_lens(None)
    r.set_moments(False)
    r.temporal_reset()


@pytest.mark.parametrize("lens_name", ["fov", "both", "aperture"])
@pytest.mark.parametrize("name,K,w,h", [(n, K, W, H) for n in ("room", "open", "textured") for K in (1, 2, 4)] + [("room", 4, 37, 23), ("textured", 2, 37, 23)])
def test_guides_and_counts_under_a_lens_equal_the_cpu_chain(lens_off, rpt, oracle, name, K, w, h, lens_name):
    """rpt_read_guides and rpt_guides_info_get == the CPU chain over the lens-centre rays, bit for bit; "aperture" (the reference's field of view): the
    bytes of the chain without a lens"""
    r = lens_off
    prepare_under(r, rpt, name, K, lens_name, w, h)
    want, want_info = cpu_chain_under(oracle, name, K, lens_name, w, h)
    got = r.guides()
    check_guides(got, want, f"{name} K={K} {w}x{h} under {lens_name}")
    check_info(r.guides_info(), want_info, K)
    assert want_info["pixels_through_glass"] > 0 and want_info["rounds"] >= 2
    pinhole, pinhole_info = cpu_chain(oracle, name, K, w, h)
    if lens_name == "aperture":
        check_guides(got, pinhole, "the aperture must not enter")
        check_info(r.guides_info(), pinhole_info, K)
    else:
        assert not same_bits(got["depth"], pinhole["depth"])          # (the field of view is there)


@pytest.mark.parametrize("lens_name", ["fov", "both"])
def test_a_pixel_that_sees_no_glass_has_the_first_hit_record_under_the_lens(lens_off, rpt, oracle, lens_name):
    """K = 0 under the lens (the first-hit build, its own launch of the lens rays) against K = 4 (the chain build's): equal byte for byte wherever the first
    hit under the lens is no glass; and K = 0 is the CPU chain of budget 0 over the lens-centre rays in kind and depth"""
    r = lens_off
    for name in ("room", "textured"):
        world, rec, cfg = prepare_under(r, rpt, name, 0, lens_name)
        off = r.guides()
        assert r.guides_info()["rounds"] == 1
        r.set_guides_through_glass(4)
        on = r.guides()
        check_guides(on, cpu_chain_under(oracle, name, 4, lens_name)[0], f"{name} K=4 under {lens_name}")
        zero, _ = cpu_chain_under(oracle, name, 0, lens_name)
        assert same_bits(off["kind"], zero["kind"]) and same_bits(off["depth"], zero["depth"])
        untouched = same = (on["depth"].view(np.uint32) == off["depth"].view(np.uint32)) & (on["kind"] == off["kind"])
        for k in ("albedo", "normal", "position"):
            same = same & (on[k].view(np.uint32) == off[k].view(np.uint32)).all(axis=-1)
        rays = lens_ref.centre_rays(cfg, lens_ref.LENSES[lens_name][0], oracle)
        first_material = world.indices[oracle.trace_rays(oracle.scene(world), 0, *rays)[1]]["material"].reshape(H, W)
        no_glass = (rec["model"][first_material] != model_scenes.MODEL_GLASS) | (off["kind"] != 1)
        assert no_glass.sum() > 1000 and np.all(same[no_glass]) and not np.all(untouched)


def test_a_changed_lens_rebuilds_the_guides_while_the_chain_is_on(lens_off, rpt, hipmod):
    r = lens_off
    prepare_under(r, rpt, "room", 2, "fov", spp=1)
    rebuilt = lambda: r.denoise(with_report=True)[1]["guides_rebuilt"]
    assert rebuilt() == 1 and rebuilt() == 0
    r.set_camera_lens(lens_ref.lens("fov"))                             # the same record again: nothing is stale
    assert rebuilt() == 0
    r.set_camera_lens(lens_ref.lens("both"))
    assert rebuilt() == 1 and rebuilt() == 0
    r.set_camera_lens(lens_ref.lens("both"))
    assert rebuilt() == 0
    r.set_camera_lens(lens_ref.lens("narrow"))
    assert rebuilt() == 1
    r.set_camera_lens(None)
    assert rebuilt() == 1 and rebuilt() == 0


@pytest.mark.parametrize("lens_name", ["fov", "both"])
def test_the_filters_under_a_lens_equal_their_host_builds_on_the_chains_guides(lens_off, rpt, hipmod, oracle, lens_name):
    """rpt_denoise and rpt_denoise_variance == their host builds fed the CPU chain's guides and sigma_plane * tan_half_fov; rpt_denoise_temporal under a
    field of view is still refused by name"""
    K = 2
    r = lens_off
    tan_half = F(lens_ref.LENSES[lens_name][0])
    r.set_moments(True)
    prepare_under(r, rpt, "room", K, lens_name, spp=SPP)
    g, _ = cpu_chain_under(oracle, "room", K, lens_name)
    planes = (g["albedo"], g["normal"], g["position"], g["depth"], g["kind"])
    mean, moments = mean_of(r), r.read_moments()
    for it, sp in [(2, 1.0), (3, 0.37)]:
        dev = r.denoise(params=hipmod.denoise_params(iterations=it, sigma_plane=sp))
        assert same_image(dev, hipmod.denoise_host(mean, *planes, hipmod.denoise_params(iterations=it, sigma_plane=float(F(sp) * tan_half)), 0)), (it, sp)
        assert not same_image(dev, hipmod.denoise_host(mean, *planes, hipmod.denoise_params(iterations=it, sigma_plane=sp), 0))      # (the factor is there)
        rgb, var = r.denoise_variance(params=hipmod.denoise_var_params(iterations=it, sigma_plane=sp, sigma_variance=4.0))
        want = hipmod.denoise_variance_host(mean, *planes, moments, hipmod.denoise_var_params(iterations=it, sigma_plane=float(F(sp) * tan_half), sigma_variance=4.0), 0)
        assert same_image(rgb, want[0]) and same_image(var, want[1]), (it, sp)
    with pytest.raises(hipmod.RptError) as e:
        r.denoise_temporal()
    assert e.value.code == -1 and "rpt_denoise_temporal" in str(e.value) and "field of view" in str(e.value)


def test_temporal_under_an_aperture_alone_equals_its_host_build(lens_off, rpt, hipmod, oracle):
    """an aperture with the reference's field of view: the projection is the reference camera's, the guides are the chain's without a lens (K = 2)"""
    K = 2
    r = lens_off
    r.set_moments(True)
    r.temporal_reset()
    _, _, cfg = prepare_under(r, rpt, "room", K, "aperture", spp=SPP)
    g, _ = cpu_chain(oracle, "room", K)
    tp = hipmod.temporal_params(sigma_variance=4.0)
    want = hipmod.denoise_temporal_host(mean_of(r), g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], r.read_moments(), cfg, None, tp, 0)
    rgb, var, hist, rep = r.denoise_temporal(params=tp, with_report=True)
    assert same_image(rgb, want["rgb"]) and same_image(var, want["variance"]) and same_image(hist, want["history"]) and rep["pixels_with_history"] == 0
