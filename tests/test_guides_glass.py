"""Guides that follow glass (rpt_set_guides_through_glass; csrc/k_guides_glass.h dn_glass_step) without a GPU: the host build of the step
(hipmod.glass_step_host), chained with the oracle's nearest-hit walk, against the numpy restatement of tests/guides_glass_ref.py word for word on the
material-model scenes; the all-PBR case against the first-hit guides; hand-built cases of the step; the hook's refusals; and what the guide of a pixel that
looks through the room's pane says."""
import numpy as np
import pytest

import denoise_ref
import guides_glass_ref as ref
import model_scenes

F = np.float32
W, H = 80, 72
PLANES = ("albedo", "normal", "depth", "position", "kind")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    return a.shape == b.shape and np.array_equal(a, b)


def host_step(hipmod, world, models, K):
    return lambda *a: hipmod.glass_step_host(world, models, K, *a)


_chains = {}


def chains(hipmod, oracle, name, K, w=W, h=H, models="scene"):
    """(the hook's guides and counts, the restatement's) of a scene, computed once per process"""
    key = (name, K, w, h, models if isinstance(models, str) else "pbr")
    if key not in _chains:
        world, rec, skybox, _ = model_scenes.scene(name)
        rec = rec if isinstance(models, str) else models
        cfg = model_scenes.config(name, 0, w, h)
        sc = oracle.scene(world, skybox_f32=skybox)
        _chains[key] = (ref.guides(world, rec, K, cfg, oracle, sc, step_fn=host_step(hipmod, world, rec, K)), ref.guides(world, rec, K, cfg, oracle, sc))
    return _chains[key]


@pytest.mark.parametrize("K", [1, 2, 4, 8])
@pytest.mark.parametrize("name", ["room", "open", "textured"])
def test_host_step_equals_the_restatement_word_for_word(hipmod, oracle, name, K):
    (got, got_info), (want, want_info) = chains(hipmod, oracle, name, K)
    for k in PLANES:
        assert same_bits(got[k], want[k]), f"{name} K={K}: {k} differs in {np.count_nonzero(got[k] != want[k])} entries"
    assert got_info == want_info
    assert want_info["pixels_through_glass"] > 0 and want_info["rounds"] >= 2, "the scene shows glass"
    assert want_info["rays"][0] == W * H and all(a >= b for a, b in zip(want_info["rays"], want_info["rays"][1:]))
    assert set(np.unique(want["kind"])) <= {0, 1, 2}


@pytest.mark.parametrize("name", ["room", "open", "textured"])
def test_all_pbr_records_give_the_first_hit_guides(hipmod, oracle, name):
    """K > 0 with every record PBR (and with no records at all) ends every chain in the first round: the chain's planes are those of K = 0, byte for byte, and
    the first-hit restatement's kinds and depths"""
    world, rec, skybox, _ = model_scenes.scene(name)
    pbr = model_scenes.records([model_scenes.MODEL_PBR] * len(rec))
    (got, info), (want, _) = chains(hipmod, oracle, name, 4, models=pbr)
    cfg = model_scenes.config(name, 0, W, H)
    sc = oracle.scene(world, skybox_f32=skybox)
    none, info_none = ref.guides(world, None, 4, cfg, oracle, sc, step_fn=host_step(hipmod, world, None, 4))
    zero, _ = ref.guides(world, rec, 0, cfg, oracle, sc, step_fn=host_step(hipmod, world, rec, 0))
    first = denoise_ref.guides(world, cfg, oracle, sc)
    for k in PLANES:
        assert same_bits(got[k], want[k]) and same_bits(got[k], none[k]) and same_bits(got[k], zero[k]), k
    assert info["rounds"] == info_none["rounds"] == 1 and info["pixels_through_glass"] == 0 and info["pixels_exhausted"] == 0
    assert same_bits(got["kind"], first["kind"]) and same_bits(got["depth"], first["depth"])
    assert np.abs(got["normal"] - first["normal"]).max() <= 1e-6 and np.abs(got["albedo"] - first["albedo"]).max() <= 1e-6


# ---- hand-built cases: a big glass quad in the plane z = 1 (normal towards -z, tint TINT, ior 1.5), and whatever a case puts behind it -----------------------
TINT = (0.5, 0.75, 0.25)
WALL = (0.8, 0.25, 0.2)


def bench(behind=None, zero_normal=False):
    """material 0: the glass quad; material 1: `behind` = "wall" (a Lambertian quad in z = 3) or "lamp" (an emitter there)"""
    g = model_scenes._Mesh()
    g.quad([(-50, -50, 1), (50, -50, 1), (50, 50, 1), (-50, 50, 1)], (0, 0, 0) if zero_normal else (0, 0, -1), 0)
    if behind:
        g.quad([(-50, -50, 3), (50, -50, 3), (50, 50, 3), (-50, 50, 3)], (0, 0, -1), 1)
    black = (0.0, 0.0, 0.0)
    w = g.world([(0.05, 0.0, TINT, black), (1.0, 0.0, black if behind == "lamp" else WALL, (5.0, 4.0, 3.0) if behind == "lamp" else black)])
    return w, model_scenes.records([model_scenes.MODEL_GLASS, model_scenes.MODEL_LAMBERTIAN], [1.5, 0.0])


def both(hipmod, oracle, world, rec, K, ro, rd, hits=None, A=None, L=None, m=None):
    """one step of the rays through the hook and through the restatement, equal word for word -> the hook's"""
    ro, rd = np.array(ro, F).reshape(-1, 3), np.array(rd, F).reshape(-1, 3)
    n = len(ro)
    t, tri, flags = hits if hits is not None else oracle.trace_rays(oracle.scene(world), 0, ro, rd)[:3]
    A = np.ones((n, 3), F) if A is None else np.array(A, F).reshape(n, 3)
    L, m = np.zeros(n, F) if L is None else np.array(L, F), np.zeros(n, np.uint32) if m is None else np.array(m, np.uint32)
    got = hipmod.glass_step_host(world, rec, K, ro, rd, t, tri, flags, A, L, m)
    want = ref.step(world, rec, K, oracle, ro, rd, t, tri, flags, A, L, m)
    for k in want:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        if a.dtype == np.float32:
            nan = np.isnan(a)
            assert np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32)), k
        else:
            assert np.array_equal(a, b), k
    return got


def unit(v):
    v = np.array(v, np.float64)
    return (v / np.linalg.norm(v)).astype(F)


def test_step_normal_incidence_refracts_straight_on(hipmod, oracle):
    world, rec = bench("wall")
    s = both(hipmod, oracle, world, rec, 4, [(0, 0, 0)], [(0, 0, 1)])
    assert s["active"][0] and not s["exhausted"][0] and s["interfaces"][0] == 1 and s["length"][0] == F(1.0)
    assert np.allclose(s["dirs"][0], (0, 0, 1), atol=1e-6) and np.allclose(s["origins"][0], (0, 0, 1.001), atol=1e-6)
    assert same_bits(s["albedo_product"][0], np.array(TINT, F))                            # refracted: A = 1 * tint, exact


def test_step_reflects_inside_at_a_grazing_angle(hipmod, oracle):
    """from behind the quad (the side its normal points away from: inside), 84 degrees off the normal: Schlick's term is 0.6 > 0.5"""
    world, rec = bench()
    rd = unit((1.0, 0.0, -0.1))
    s = both(hipmod, oracle, world, rec, 4, [(0, 0, 2)], [rd], A=[(0.3, 0.4, 0.5)], L=[2.5], m=[1])
    assert s["active"][0] and s["interfaces"][0] == 2
    assert same_bits(s["albedo_product"][0], np.array((0.3, 0.4, 0.5), F))                # reflected: A unchanged
    assert np.allclose(s["dirs"][0], (rd[0], 0.0, -rd[2]), atol=1e-6) and s["dirs"][0][2] > 0
    assert s["length"][0] > F(2.5)


def test_step_refraction_with_the_clamped_root(hipmod, oracle):
    """inside, c = 0.3: 1 + eta (c c - 1) = -0.365 with the reference's un-squared eta = 1.5, clamped to 0 before the root, and Schlick's term is 0.2: the
    direction is normalize(eta c n' - eta view), as the tracer's"""
    world, rec = bench()
    rd = unit((np.sqrt(1 - 0.09), 0.0, -0.3))
    s = both(hipmod, oracle, world, rec, 4, [(0, 0, 2)], [rd], A=[(1, 1, 1)])
    assert s["active"][0] and same_bits(s["albedo_product"][0], np.array(TINT, F))
    c = F(0.3)
    assert F(1.0) + F(1.5) * (c * c - F(1.0)) < 0
    expect = unit(1.5 * 0.3 * np.array((0, 0, 1.0)) - 1.5 * (-rd.astype(np.float64)))
    assert np.allclose(s["dirs"][0], expect, atol=1e-6)


def test_step_zero_normal_ends_the_chain_on_the_glass(hipmod, oracle):
    world, rec = bench(zero_normal=True)
    s = both(hipmod, oracle, world, rec, 4, [(0, 0, 0)], [(0, 0, 1)], A=[(0.5, 0.5, 0.5)])
    assert not s["active"][0] and s["exhausted"][0] and s["kind"][0] == 1 and np.all(s["normal"][0] == 0)
    assert same_bits(s["albedo"][0], np.array((0.5, 0.5, 0.5), F) * np.array(TINT, F))


def test_step_direction_that_is_not_finite_counts_as_an_exhausted_budget(hipmod, oracle):
    """a hand-fed hit at t = 0 of a ray whose direction is (0, 0, 3e38): c c overflows, inf - inf is the coefficient"""
    world, rec = bench()
    hits = (np.zeros(1, F), np.zeros(1, np.uint32), np.ones(1, np.uint32))
    s = both(hipmod, oracle, world, rec, 4, [(0, 0, 1)], [(0, 0, 3e38)], hits=hits)
    assert not s["active"][0] and s["exhausted"][0] and s["kind"][0] == 1 and s["interfaces"][0] == 0
    assert np.allclose(s["normal"][0], (0, 0, -1)) and same_bits(s["albedo"][0], np.array(TINT, F))


def test_chain_emitter_and_wall_behind_the_pane(hipmod, oracle):
    for behind, kind, albedo in (("lamp", 2, np.array(TINT, F)), ("wall", 1, np.array(TINT, F) * np.array(WALL, F))):
        world, rec = bench(behind)
        ro, rd = np.array([(0, 0, 0)], F), unit((0.1, 0.2, 1.0)).reshape(1, 3)
        planes, info = ref.run_chains(host_step(hipmod, world, rec, 4), ref.oracle_walk(oracle, oracle.scene(world)), ro, rd, 4)
        want, _ = ref.run_chains(lambda *a: ref.step(world, rec, 4, oracle, *a), ref.oracle_walk(oracle, oracle.scene(world)), ro, rd, 4)
        assert all(same_bits(planes[k], want[k]) for k in PLANES)
        assert planes["kind"][0] == kind and same_bits(planes["albedo"][0], albedo)       # an emitter's a is (1, 1, 1): the albedo is A
        assert info["rounds"] == 2 and info["rays"][:3] == [1, 1, 0] and info["pixels_through_glass"] == 1 and info["pixels_exhausted"] == 0
        assert planes["depth"][0] > 3.0 and np.allclose(planes["normal"][0], (0, 0, -1), atol=1e-6)


def test_chain_miss_behind_glass(hipmod, oracle):
    world, rec = bench()
    ro, rd = np.array([(0, 0, 0)], F), np.array([(0, 0, 1)], F)
    planes, info = ref.run_chains(host_step(hipmod, world, rec, 4), ref.oracle_walk(oracle, oracle.scene(world)), ro, rd, 4)
    assert planes["kind"][0] == 0 and np.all(planes["normal"][0] == 0) and same_bits(planes["albedo"][0], np.array(TINT, F))
    assert planes["depth"][0] == F(1.0) + F(1e6) and info["pixels_through_glass"] == 1
    assert same_bits(planes["position"][0], (ro + rd * planes["depth"][0])[0])


def test_chain_budget_of_one_ends_inside_the_sphere(hipmod, oracle):
    (got, info), _ = chains(hipmod, oracle, "open", 1)
    (deep, deep_info), _ = chains(hipmod, oracle, "open", 8)
    assert info["rounds"] == 2 and info["pixels_exhausted"] > 0 and info["pixels_exhausted"] <= info["rays"][1]
    world, rec, skybox, _ = model_scenes.scene("open")
    cfg = model_scenes.config("open", 0, W, H)
    first = denoise_ref.guides(world, cfg, oracle, oracle.scene(world, skybox_f32=skybox))
    sphere = world.indices[oracle.trace_rays(oracle.scene(world), 0, *denoise_ref.camera_rays(cfg, oracle))[1]]["material"].reshape(H, W) == 1
    sphere &= first["kind"] == 1
    assert sphere.sum() == info["rays"][1]                                                 # every ray that met the sphere went on ...
    inside = sphere & (got["kind"] == 1) & (got["depth"] < 100)
    assert 0.8 * sphere.sum() < info["pixels_exhausted"] <= inside.sum()                   # ... and, but for the rim's reflections, ended on glass again
    assert np.all(got["depth"][sphere] > first["depth"][sphere])
    assert deep_info["pixels_exhausted"] < info["pixels_exhausted"] and len(np.unique(deep["kind"][sphere])) > 1      # with budget the ground and the sky show


def test_hook_refusals(hipmod, oracle):
    world, rec = bench("wall")
    one = lambda **kw: hipmod.glass_step_host(world, rec, kw.get("K", 4), [(0, 0, 0)], [(0, 0, 1)], [1.0], [kw.get("tri", 0)], [1], [(1, 1, 1)], [0.0], [0])
    assert one()["active"][0]
    for kw in ({"K": 9}, {"tri": len(world.indices)}):
        with pytest.raises(hipmod.RptError) as e:
            one(**kw)
        assert e.value.code == -1
    tw, trec, _, _ = model_scenes.scene("textured")

    class NoAtlas:
        per_vertex, indices, materials, atlas = tw.per_vertex, tw.indices, tw.materials, None
    with pytest.raises(hipmod.RptError) as e:
        hipmod.glass_step_host(NoAtlas, trec, 4, [(0, 0, 0)], [(0, 0, 1)], [1.0], [0], [1], [(1, 1, 1)], [0.0], [0])
    assert e.value.code == -1 and "atlas" in str(e.value)


def test_a_pixel_through_the_rooms_pane_carries_the_wall_behind_it(hipmod, oracle):
    """first hit: the pane (material 4); the chain crosses its two faces and ends on the Lambertian wall x = -3 (material 1) or the grey back wall (material 0)"""
    world, rec, _, _ = model_scenes.scene("room")
    cfg = model_scenes.config("room", 0, W, H)
    sc = oracle.scene(world)
    ro, rd = denoise_ref.camera_rays(cfg, oracle)
    first_material = world.indices[oracle.trace_rays(sc, 0, ro, rd)[1]]["material"].reshape(H, W)
    first = denoise_ref.guides(world, cfg, oracle, sc)
    (g, info), _ = chains(hipmod, oracle, "room", 4)
    pane = (first_material == 4) & (first["kind"] == 1)
    assert pane.sum() > 100
    tint, red = world.materials["albedo"][4, :3].astype(F), world.materials["albedo"][1, :3].astype(F)
    on_red = pane & (g["interfaces"] == 2) & (g["kind"] == 1) & (np.abs(g["normal"] - np.array((1, 0, 0), F)).max(axis=-1) < 1e-6)
    assert on_red.sum() > 50, "pixels through the pane that end on the wall x = -3"
    assert np.all(np.abs(first["normal"][on_red][:, 0]) < 0.5)                              # (the first-hit normal there is the pane's)
    expect = (tint * tint) * red                                                            # ((1 * tint) * tint) * wall, the restatement's order
    assert np.all(g["albedo"][on_red].view(np.uint32) == expect.view(np.uint32))
    assert same_bits(first["albedo"][on_red], np.broadcast_to(tint, first["albedo"][on_red].shape))
    assert np.all(g["depth"][on_red] > first["depth"][on_red])
    # the position lies on the pixel's primary ray at distance L: it IS ro0 + rd0 * L
    assert same_bits(g["position"], (ro + rd * g["depth"].reshape(-1, 1)).astype(F).reshape(H, W, 3))
    along = g["position"][on_red] - ro.reshape(H, W, 3)[on_red]
    assert np.allclose(np.linalg.norm(along.astype(np.float64), axis=-1), g["depth"][on_red], rtol=1e-5)
    assert info["pixels_through_glass"] >= pane.sum()


@pytest.mark.parametrize("name", ["room", "open", "textured"])
def test_the_chain_over_lens_centre_rays_at_tan_half_1_is_the_chain(hipmod, oracle, name):
    """guides_glass_ref.guides takes its primary rays as an argument: handed lens_ref.centre_rays at tan_half_fov 1 — the restatement of
    k_dn_camera_rays_lens under the reference's field of view — it is the existing chain, byte for byte, counts included"""
    import lens_ref
    world, rec, skybox, _ = model_scenes.scene(name)
    cfg = model_scenes.config(name, 0, W, H)
    _, (want, want_info) = chains(hipmod, oracle, name, 4)
    got, info = ref.guides(world, rec, 4, cfg, oracle, oracle.scene(world, skybox_f32=skybox), rays=lens_ref.centre_rays(cfg, 1.0, oracle))
    for k in PLANES + ("interfaces",):
        assert same_bits(got[k], want[k]), k
    assert info == want_info


def test_a_pixel_through_the_rooms_pane_under_a_field_of_view(hipmod, oracle):
    """the pane's semantics under the lens "fov" (tan_half_fov 0.6): the chain starts from the rays through the LENS CENTRE, so a pixel that looks through
    the pane carries the normal of the wall behind it and a position on ITS lens-centre primary ray — not on the reference camera's ray of that pixel"""
    import lens_ref
    tan_half = lens_ref.LENSES["fov"][0]
    world, rec, _, _ = model_scenes.scene("room")
    cfg = model_scenes.config("room", 0, W, H)
    sc = oracle.scene(world)
    ro, rd = lens_ref.centre_rays(cfg, tan_half, oracle)
    pin_ro, pin_rd = denoise_ref.camera_rays(cfg, oracle)
    assert same_bits(ro, pin_ro) and not same_bits(rd, pin_rd)
    first_material = world.indices[oracle.trace_rays(sc, 0, ro, rd)[1]]["material"].reshape(H, W)
    g, info = ref.guides(world, rec, 4, cfg, oracle, sc, rays=(ro, rd))
    host, host_info = ref.guides(world, rec, 4, cfg, oracle, sc, step_fn=host_step(hipmod, world, rec, 4), rays=(ro, rd))
    assert all(same_bits(g[k], host[k]) for k in PLANES) and info == host_info           # the host build of the step over the same rays
    first, _ = ref.guides(world, rec, 0, cfg, oracle, sc, rays=(ro, rd))                 # K = 0: the first hit under the lens
    pane = (first_material == 4) & (first["kind"] == 1)
    assert pane.sum() > 100
    tint, red = world.materials["albedo"][4, :3].astype(F), world.materials["albedo"][1, :3].astype(F)
    on_red = pane & (g["interfaces"] == 2) & (g["kind"] == 1) & (np.abs(g["normal"] - np.array((1, 0, 0), F)).max(axis=-1) < 1e-6)
    assert on_red.sum() > 50, "pixels through the pane that end on the wall x = -3"
    assert np.all(np.abs(first["normal"][on_red][:, 0]) < 0.5)                              # (the first-hit normal there is the pane's)
    expect = (tint * tint) * red
    assert np.all(g["albedo"][on_red].view(np.uint32) == expect.view(np.uint32))
    assert np.all(g["depth"][on_red] > first["depth"][on_red])
    assert same_bits(g["position"], (ro + rd * g["depth"].reshape(-1, 1)).astype(F).reshape(H, W, 3))
    assert not same_bits(g["position"], (pin_ro + pin_rd * g["depth"].reshape(-1, 1)).astype(F).reshape(H, W, 3))
    # a narrower field of view magnifies: the pane covers more pixels than under the reference camera
    (pin, _), _ = chains(hipmod, oracle, "room", 4)
    pin_first = world.indices[oracle.trace_rays(sc, 0, pin_ro, pin_rd)[1]]["material"].reshape(H, W)
    assert pane.sum() > (pin_first == 4).sum() and not same_bits(g["depth"], pin["depth"])
    assert info["pixels_through_glass"] >= pane.sum()


def test_the_recommended_budget_is_the_kept_grids_minimum(hipmod):
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r20_glass_guides_quality.txt")).read()
    m = re.search(r"lowest summed \(a\) of K = 2, 4, 8 over the two shipped-default filters: K = (\d)", text)
    assert m and int(m.group(1)) == hipmod.GUIDES_THROUGH_GLASS and 1 <= hipmod.GUIDES_THROUGH_GLASS <= hipmod.GUIDES_MAX_INTERFACES
