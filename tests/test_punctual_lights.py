"""Punctual lights without a GPU (include/rpt/rpt.h rpt_set_punctual_lights): the bit-exact restatement tests/lights_oracle against the volume restatement
where there are no lights, the arithmetic of csrc/k_punctual.h in the host build against a numpy float32 restatement, closed forms on the restatement that
need no reference, the records of the binding, and the loader.  Every refusal of the setter is held here through rpt_debug_punctual_lights_check, the check the setter itself calls; the
refusals on a live context, a call before a scene and the setter / getter round trip need a context, which needs a device: those are in
tests/test_gpu_punctual_lights.py.  The restatement's mode for RPT_SHADOW_SEGMENT is held to tools/anyhit_order_sim.cpp ray by ray."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lens_ref
import lights_ref
import model_scenes
import scenes
import volume_ref

W, H = 32, 24
F = np.float32
BOUND = 8 * 2.0 ** -24


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("lens_name", [None, "both"])
@pytest.mark.parametrize("nee", [0, 1, 2])
@pytest.mark.parametrize("name", ["room", "textured"])
def test_without_lights_the_restatement_is_the_volume_restatement(rpt, oracle, name, nee, lens_name):
    """no lights: accumulators, rng and counters of volume_lens_trace_cpu word for word, with and without a lens; with nee 0 the lights change nothing either"""
    spp = 2
    w, rec, skybox, _ = model_scenes.scene(name)
    cfg = model_scenes.config(name, nee, W, H, **model_scenes.lens_overrides(nee, lens_name))
    sc, seeds, lens = oracle.scene(w, skybox_f32=skybox), rpt.blue_noise_seeds(W, H), lens_ref.lens(lens_name)
    vols = volume_ref.volumes(name)
    ref, ref_rng, ref_st = volume_ref.volume_lens_trace_cpu(cfg, sc, rec, vols, lens, seeds, spp)
    for lts in (None, lights_ref.lights(name)) if nee == 0 else (None,):
        acc, rng, st = lights_ref.lights_trace_cpu(cfg, sc, rec, vols, lens, lts, lights_ref.SHARE, seeds, spp)
        assert np.array_equal(words(acc), words(ref))
        assert np.array_equal(rng, ref_rng)
        assert (st.samples, st.extension_rays, st.shadow_rays, st.sky_evals, st.light_index_clamped, st.shadow_rays_zero_term, st.segments_absorbed) == \
               (ref_st.samples, ref_st.extension_rays, ref_st.shadow_rays, ref_st.sky_evals, ref_st.light_index_clamped, ref_st.shadow_rays_zero_term,
                ref_st.segments_absorbed)
        assert st.punctual_picks == 0


def test_the_host_build_of_punctual_sample_is_its_float32_restatement(hipmod):
    cases = lights_ref.sample_inputs()
    assert len(cases[-1][3]) == 500
    for lts, q, hits, l1 in cases:
        got, want = hipmod.debug_punctual_sample_host(lts, q, hits, l1), lights_ref.punctual_sample_numpy(lts, q, hits, l1)
        assert np.array_equal(got[0], want[0]), (got[0], want[0])
        for g, w_ in zip(got[1:], want[1:]):
            assert lights_ref.same_bits_or_both_nan(g, w_), np.argwhere(words(g) != words(w_))
    j, L, max_t, E, pdf = hipmod.debug_punctual_sample_host(*cases[0])
    assert j.tolist() == [2, 2] and pdf[0] == F(0.5) / F(3)                                  # l1 just below q: the last light; pick pdf q / n
    j, _, _, _, pdf = hipmod.debug_punctual_sample_host(*cases[1])
    assert j.tolist() == [0, 2, 2] and pdf[0] == F(1) / F(3)                                 # q = 1
    _, L, max_t, E, _ = hipmod.debug_punctual_sample_host(*cases[2])
    assert np.isnan(L).all() and np.isinf(E).all() and max_t[0] == F(0) - F(0.001) * F(2)   # the light at the hit: L = 0 / 0, E = I / 0; the surface's pdf of a NaN direction is 0
    _, L, max_t, E, _ = hipmod.debug_punctual_sample_host(*cases[3])
    assert L[0].tolist() == [0.0, -1.0, 0.0] and max_t[0] == F(1e6) and E[0].tolist() == [1.0, 2.0, 3.0]       # directional: towards -direction, as given
    _, _, _, E, _ = hipmod.debug_punctual_sample_host(*cases[4])
    assert not E[0].any() and not E[3].any()                                                  # on the outer cone and outside it: exactly 0
    assert E[2, 0] == F(4) * (F(1) / (F(2) * F(2)))                                           # on the axis: intensity / d^2
    d2 = F(4) + F(2.0 * np.tan(np.radians(30.0))) ** 2
    assert abs(float(E[1, 0]) / (4.0 / float(d2)) - 1.0) < 4e-6                               # on the inner cone: the full intensity (a = 1 within rounding)


def test_the_records_of_the_binding_are_the_headers(hipmod):
    dt = hipmod.PUNCTUAL_LIGHT_DTYPE
    assert dt.itemsize == 64 and dt == lights_ref.PUNCTUAL_LIGHT_DTYPE
    assert [dt.fields[k][1] for k in ("type", "position", "direction", "intensity", "angle_scale", "angle_offset", "reserved")] == [0, 4, 16, 28, 40, 44, 48]
    p = hipmod.point_light((1, 2, 3), (4, 5, 6))
    s = hipmod.spot_light((2.0, 3.2, 1.0), (-1.5, -3.2, 1.5), (20.0, 20.0, 25.0), 20.0, 35.0)
    d = hipmod.directional_light((0.3, -1.0, 0.4), (0.5, 0.5, 0.4))
    assert p["type"][0] == 0 and p["position"][0].tolist() == [1, 2, 3] and p["intensity"][0].tolist() == [4, 5, 6] and not p["direction"].any()
    room = lights_ref.lights("room")
    assert s.tobytes() == room[1:2].tobytes() and d.tobytes() == room[2:3].tobytes()           # normalised in float64, rounded once: the tests' own records
    assert abs(float(np.sum(s["direction"].astype(np.float64) ** 2)) - 1.0) < 1e-6
    ci, co = np.cos(np.radians(20.0)), np.cos(np.radians(35.0))
    assert s["angle_scale"][0] == F(1.0 / (ci - co)) and s["angle_offset"][0] == F(-co / (ci - co))
    assert hipmod.spot_light((0, 0, 0), (0, 0, 1), 1.0, 10.0, 10.0)["angle_scale"][0] == F(1000.0)       # glTF's max(0.001, .)
    assert hipmod.punctual_lights(p, s, d).shape == (3,) and hipmod.punctual_lights().shape == (0,)
    with pytest.raises(ValueError):
        hipmod.directional_light((0, 0, 0), 1.0)


# ---- closed forms: a Lambertian floor seen from straight above, one bounce, nee 1, a black image sky ----------------------------------------------------------
ALBEDO = (0.6, 0.5, 0.4)
CAM_Y = 3.0
_floor = {}


def _floor_scene(oracle, occluder):
    if occluder not in _floor:
        g = model_scenes._Mesh()
        g.quad([(-40, 0, -40), (-40, 0, 40), (40, 0, 40), (40, 0, -40)], (0, 1, 0), 0)
        if occluder:                      # one unit above the floor, symmetric in z; lit from the -x side it shades x 0.5 .. 1.5 of the floor
            g.quad([(-0.5, 1, -0.4), (-0.5, 1, 0.4), (0.5, 1, 0.4), (0.5, 1, -0.4)], (0, 1, 0), 0)
        w = g.world([(1.0, 0.0, ALBEDO, (0.0, 0.0, 0.0))])
        sky = np.zeros((4, 8, 4), F)
        sky[..., 3] = 1.0
        _floor[occluder] = (w, model_scenes.records([model_scenes.MODEL_LAMBERTIAN]), oracle.scene(w, skybox_f32=sky))
    return _floor[occluder]


def _floor_samples(rpt, oracle, lts, occluder=False, spp=3):
    w, rec, sc = _floor_scene(oracle, occluder)
    cfg = rpt.default_config(W, H, nee=1, max_bounces=1, min_bounces=0, has_skybox=1, cam_position=(0.0, CAM_Y, 0.0, 0.0),
                             cam_rotation=(float(F(np.pi / 2)), 0.0, 0.0, 0.0))
    rng = rpt.blue_noise_seeds(W, H)
    out, starts = [], []
    for _ in range(spp):
        starts.append(np.ascontiguousarray(rng).copy())
        one, picks = lights_ref.lights_trace_samples(cfg, sc, rec, None, None, lts, 0.5, rng)
        assert (picks == 1).all()                                  # no emissive triangle: q = 1, every sample's one NEE evaluation picks a punctual light
        _, rng, _ = lights_ref.lights_trace_cpu(cfg, sc, rec, None, None, lts, 0.5, rng, 1)
        out.append(one)
    return np.stack(out).astype(np.float64), np.stack(starts)


def _floor_x_range():
    """the floor x a pixel column can see, whatever the jitter: the camera looks straight down from CAM_Y with a 90 degree horizontal field, and a rotation
    about the x axis leaves x alone: x = CAM_Y * uv.x up to the rounding of cos(pi / 2)"""
    x = np.arange(W)
    return CAM_Y * (x / W * 2 - 1) - 1e-3, CAM_Y * ((x + 1) / W * 2 - 1) + 1e-3


def _floor_z_abs_range():
    """... and |z| of a pixel row: |z| = CAM_Y * |uv.y|, uv.y = (1 - (y + j) / H * 2... ) * H / W"""
    y = np.arange(H)
    a, b = (1 - y / H * 2) * H / W * CAM_Y, (1 - (y + 1) / H * 2) * H / W * CAM_Y
    lo = np.where(a * b <= 0, 0.0, np.minimum(np.abs(a), np.abs(b)))
    return lo - 1e-3, np.maximum(np.abs(a), np.abs(b)) + 1e-3


def test_under_a_directional_light_every_floor_sample_is_albedo_over_pi_e_cos(rpt, oracle):
    direction, E = np.array([0.6, -0.8, 0.0]), np.array([1.5, 2.0, 0.75])
    rad, _ = _floor_samples(rpt, oracle, lights_ref.directional(direction, E))
    want = np.array(ALBEDO) / np.pi * E * 0.8
    assert np.all(np.abs(rad - want) <= BOUND * want), np.abs(rad / want - 1).max() / 2.0 ** -24


def test_behind_an_occluding_quad_the_floor_is_black(rpt, oracle):
    """lit along (1, -1, 0): the quad over x -0.5 .. 0.5 at height 1 shades x 0.5 .. 1.5, |z| < 0.4 of the floor; the camera sees that strip beside the quad"""
    rad, _ = _floor_samples(rpt, oracle, lights_ref.directional((1.0, -1.0, 0.0), (1.0, 1.0, 1.0)), occluder=True)
    x0, x1 = _floor_x_range()
    z0, z1 = _floor_z_abs_range()
    shaded = ((x0 > 0.8) & (x1 < 1.45))[None, :] & (z1 < 0.35)[:, None]        # (x > 0.75: past where the quad itself hides the floor, 0.5 * 3 / 2)
    lit = ((x0 > 1.6) | (x1 < -0.8))[None, :] & np.ones(H, bool)[:, None]
    assert shaded.sum() >= 4 and lit.sum() > 100
    assert not rad[:, shaded].any()                                            # exactly 0
    assert (rad[:, lit] > 0).all()


def test_outside_a_spots_outer_cone_the_floor_is_black(rpt, oracle):
    """a spot straight down from height 2, outer cone 30 degrees: its disk on the floor has radius 2 tan 30 = 1.1547"""
    rad, _ = _floor_samples(rpt, oracle, lights_ref.spot((0.0, 2.0, 0.0), (0.0, -1.0, 0.0), (3.0, 3.0, 3.0), 15.0, 30.0))
    x0, x1 = _floor_x_range()
    z0, z1 = _floor_z_abs_range()
    xmin = np.where(x0 * x1 <= 0, 0.0, np.minimum(np.abs(x0), np.abs(x1)))
    xmax = np.maximum(np.abs(x0), np.abs(x1))
    outside = np.hypot(xmin[None, :], np.maximum(z0, 0)[:, None]) > 1.16
    inside = np.hypot(xmax[None, :], z1[:, None]) < 2 * np.tan(np.radians(15.0))
    assert outside.sum() > 100 and inside.sum() >= 4
    assert not rad[:, outside].any()                                           # exactly 0
    assert (rad[:, inside] > 0).all()


def test_a_point_light_at_twice_the_height_gives_a_quarter(rpt, oracle):
    """the light straight above a sample's hit point, at height h and at 2 h: cos = 1, the term is albedo / pi * I / h^2.  The hit point comes from the sample's
    jitter (the first two draws) in float64; what it misses of the restatement's f32 hit, some 1e-6, enters the term squared: far below the bound."""
    px, py = 20, 9
    seeds = rpt.blue_noise_seeds(W, H).reshape(H, W)
    n, offset = int(seeds[py, px]["n"]), int(seeds[py, px]["offset"])
    jx, jy = oracle.lds(n, 1, offset)[1], oracle.lds(n, 2, offset)[1]
    ux, uy = (px + jx) / W * 2 - 1, (1 - (py + jy) / H * 2) * H / W
    angle = float(F(np.pi / 2))
    c, s = np.cos(angle), np.sin(angle)
    d = np.array([ux, c * uy - s, s * uy + c])                    # rotation_x(angle) * (ux, uy, 1), not normalised
    hit = np.array([0.0, CAM_Y, 0.0]) + d * (CAM_Y / -d[1])
    intensity, h = np.array([5.0, 4.0, 3.0]), 1.25
    terms = []
    for height in (h, 2 * h):
        rad, _ = _floor_samples(rpt, oracle, lights_ref.point((hit[0], height, hit[2]), intensity), spp=1)
        terms.append(rad[0, py, px])
    want = np.array(ALBEDO) / np.pi * intensity / h ** 2
    assert np.all(np.abs(terms[0] - want) <= BOUND * want), np.abs(terms[0] / want - 1).max() / 2.0 ** -24
    assert np.all(np.abs(terms[1] - terms[0] / 4) <= BOUND * terms[0] / 4), np.abs(terms[1] * 4 / terms[0] - 1).max() / 2.0 ** -24


@pytest.mark.parametrize("nee", [1, 2])
@pytest.mark.parametrize("name", ["room", "small_room", "open", "textured"])
def test_the_scenes_pick_both_kinds_of_light(oracle, name, nee, capsys):
    """not vacuous: punctual picks in every scene, mesh picks beside them where the scene has emissive triangles, and a finite image that differs"""
    spp = 2
    acc, rng, st = lights_ref.reference(oracle, name, nee, W, H, spp)
    plain, plain_rng, plain_st = lights_ref.reference(oracle, name, nee, W, H, spp, lts=None)
    with capsys.disabled():
        print(f"\n{name} nee {nee}: {st.punctual_picks} punctual picks of {st.shadow_rays} light samples ({plain_st.shadow_rays} without lights)", end="")
    assert st.punctual_picks > 0 and np.isfinite(acc).all() and (words(acc) != words(plain)).any()
    assert np.array_equal(rng, plain_rng)
    if name == "open":
        assert plain_st.shadow_rays == 0 and st.shadow_rays == st.punctual_picks            # no emissive triangle: q = 1, and the draws are now made
    else:
        assert 0 < st.punctual_picks < st.shadow_rays


# ---- the loader ---------------------------------------------------------------------------------------------------------------------------------------------
def _lights_glb(path, with_extension=True):
    """one triangle under node 0, and under it: node 1, rotated a quarter turn about x and translated, with a spot light; node 2, scaled by 2 and translated, with
    the children node 3 (a directional light) and node 5 (the point light); node 4, which refers to the same point light once more"""
    import json
    import struct
    scenes.write_glb(str(path), [[0, 0, 0], [1, 0, 0], [0, 1, 0]], [0, 1, 2])
    if not with_extension:
        return str(path)
    data = open(path, "rb").read()
    jlen = struct.unpack_from("<I", data, 12)[0]
    doc, rest = json.loads(data[20:20 + jlen]), data[20 + jlen:]
    ref = lambda i: {"KHR_lights_punctual": {"light": i}}
    h = float(np.sqrt(0.5))
    doc["nodes"][0]["children"] = [1, 2, 4]
    doc["nodes"] += [{"translation": [1.0, 2.0, 3.0], "rotation": [h, 0.0, 0.0, h], "extensions": ref(0)},
                     {"translation": [0.0, 1.0, 0.0], "scale": [2.0, 2.0, 2.0], "children": [3, 5]},
                     {"translation": [1.0, 0.0, 0.0], "extensions": ref(1)},
                     {"translation": [5.0, 6.0, 7.0], "extensions": ref(2)},
                     {"translation": [1.0, 1.0, 1.0], "extensions": ref(2)}]
    doc["extensionsUsed"] = ["KHR_lights_punctual"]
    doc["extensions"] = {"KHR_lights_punctual": {"lights": [
        {"type": "spot", "color": [1.0, 0.5, 0.25], "intensity": 10.0, "spot": {"innerConeAngle": 0.2, "outerConeAngle": 0.5}},
        {"type": "directional", "intensity": 3.0},
        {"type": "point", "color": [0.5, 0.5, 1.0], "range": 4.0}]}}
    js = json.dumps(doc).encode()
    js += b" " * (-len(js) % 4)
    out = struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(js) + len(rest)) + struct.pack("<II", len(js), 0x4E4F534A) + js + rest
    open(path, "wb").write(out)
    return str(path)


def test_the_loader_reads_the_lights_only_when_asked(rpt, hipmod, tmp_path):
    path = _lights_glb(tmp_path / "lights.glb")
    plain, flagged = rpt.World.from_path(path), rpt.World.from_path(path, punctual_lights=True)
    assert len(plain.punctual_lights) == 0 and plain.punctual_lights.dtype == hipmod.PUNCTUAL_LIGHT_DTYPE
    got = flagged.punctual_lights
    assert got.dtype == hipmod.PUNCTUAL_LIGHT_DTYPE and not got["reserved"].any()
    assert got["type"].tolist() == [1, 2, 0, 0]                   # in walk order; the light referred to twice comes out twice
    # the spot: translated to (1, 2, 3); its -Z axis after a quarter turn about x is +Y; both swapped (x, z, y)
    assert got["position"][0].tolist() == [1.0, 3.0, 2.0]
    assert np.allclose(got["direction"][0], (0.0, 0.0, 1.0), atol=1e-6) and abs(float(np.sum(got["direction"][0].astype(np.float64) ** 2)) - 1) < 1e-6
    assert got["intensity"][0].tolist() == [10.0, 5.0, 2.5]       # color * intensity, as written
    scale = 1.0 / (np.cos(0.2) - np.cos(0.5))
    assert got["angle_scale"][0] == F(scale) and got["angle_offset"][0] == F(-np.cos(0.5) * scale)
    # the directional light under a parent scaled by 2: -Z, swapped, of unit length whatever the scale; no position
    assert got["direction"][1].tolist() == [0.0, -1.0, 0.0] and not got["position"][1].any() and got["intensity"][1].tolist() == [3.0, 3.0, 3.0]
    # the point light twice: under the scaled parent (0, 1, 0) + 2 * (1, 1, 1) = (2, 3, 2), and at (5, 6, 7); swapped; no direction; `range` is not read
    assert got["position"][2].tolist() == [2.0, 2.0, 3.0] and got["position"][3].tolist() == [5.0, 7.0, 6.0]
    assert not got["direction"][2:].any() and got["intensity"][2].tolist() == [0.5, 0.5, 1.0] and got[2]["intensity"].tobytes() == got[3]["intensity"].tobytes()
    assert not got["angle_scale"][1:].any() and not got["angle_offset"][1:].any()
    for field in ("per_vertex", "indices", "nodes", "materials", "light_pick"):      # the world itself does not depend on the flag
        assert getattr(plain, field).tobytes() == getattr(flagged, field).tobytes()
    a, b = tmp_path / "a.rptscene", tmp_path / "b.rptscene"
    plain.save(str(a)); flagged.save(str(b))
    assert a.read_bytes() == b.read_bytes()                                          # ... nor does the cache, which does not carry the lights
    assert len(rpt.World.from_cache(str(b)).punctual_lights) == 0


def test_a_file_without_the_extension_has_no_lights(rpt, tmp_path):
    path = _lights_glb(tmp_path / "plain.glb", with_extension=False)
    assert len(rpt.World.from_path(path, punctual_lights=True).punctual_lights) == 0
    assert len(rpt.World.from_path(rpt.fixture("DarkCornell.glb"), punctual_lights=True).punctual_lights) == 0


# ---- every refusal, without a device ------------------------------------------------------------------------------------------------------------------------
def test_the_host_hook_refuses_what_the_setter_refuses(hipmod):
    """rpt_debug_punctual_lights_check is the function rpt_set_punctual_lights calls before it touches its context: code and message are the setter's"""
    lts = lights_ref.lights("room")
    check = hipmod.debug_punctual_lights_check
    assert check(lts, 0.5, True) == (0, "") and check(None) == (0, "") and check(lts[:1], 0.999, True)[0] == 0

    def refused(records, share, emitters, *words):
        rc, msg = check(records, share, emitters)
        assert rc == -1 and msg.startswith("rpt_set_punctual_lights: "), (rc, msg)
        for word in words:
            assert word in msg, msg

    def with_(index, field, value):
        bad = lts.copy()
        bad[field][index] = value
        return bad

    refused(with_(1, "type", 3), 0.5, True, "record 1", "type 3")                              # a type above 2
    refused(with_(0, "type", 0xffffffff), 0.5, True, "record 0")
    for field in ("position", "direction", "intensity"):
        for value in (np.nan, np.inf, -np.inf):
            for k in range(3):
                v = [0.0, 0.0, 0.0]; v[k] = value
                refused(with_(2, field, v), 0.5, True, "record 2", "not finite")               # not finite, in any channel
    refused(with_(0, "intensity", (1.0, -0.5, 1.0)), 0.5, True, "record 0", "negative")        # a negative intensity
    refused(with_(1, "direction", (0.0, -1.01, 0.0)), 0.5, True, "record 1", "unit length")    # |len^2 - 1| > 1e-3 on a spot ...
    refused(with_(2, "direction", (0.0, 0.0, 0.0)), 0.5, True, "record 2", "unit length")      # ... and on a directional record
    assert check(with_(1, "direction", (0.0, -1.0004, 0.0)), 0.5, True)[0] == 0                # within 1e-3: used as given
    assert check(with_(0, "direction", (0.0, 5.0, 0.0)), 0.5, True)[0] == 0                    # a point light's direction is ignored
    for field in ("angle_scale", "angle_offset"):
        for value in (np.nan, np.inf, -np.inf):
            refused(with_(1, field, value), 0.5, True, "record 1", field)
    for word in range(4):
        bad = lts.copy(); bad["reserved"][2, word] = 1
        refused(bad, 0.5, True, "record 2", "reserved")                                        # reserved != 0
    for share in (0.0, 1.0, -0.5, 1.5, np.nan, np.inf):                                         # a scene with emissive triangles: (0, 1) exclusive
        refused(lts, share, True, "pick_share")
        assert check(lts, share, False)[0] == 0                                                # ... and ignored over a scene without any
        assert check(None, share, True)[0] == 0                                                # ... and with no lights
    refused(np.repeat(lts[:1], 65536), 0.5, True, "65535")
    assert check(np.repeat(lts[:1], 65535), 0.5, True)[0] == 0
    L = hipmod.lib()
    keep = np.ascontiguousarray(lts)
    msg = C.create_string_buffer(256)
    assert L.rpt_debug_punctual_lights_check(None, len(lts), 0.5, 1, msg, len(msg)) == -1 and b"NULL" in msg.value       # NULL with n != 0 ...
    assert L.rpt_debug_punctual_lights_check(hipmod.ptr(keep), 0, 0.5, 1, msg, len(msg)) == -1 and b"NULL" in msg.value  # ... and the reverse
    assert L.rpt_debug_punctual_lights_check(None, len(lts), 0.5, 1, None, 0) == -1                                      # the message is optional
    short = C.create_string_buffer(8)
    assert L.rpt_debug_punctual_lights_check(None, 1, 0.5, 1, short, len(short)) == -1 and short.value == b"rpt_set"      # truncated, terminated
    # the sampling hook takes what the setter takes
    hits, l1 = np.zeros((1, 3), F), np.full(1, 0.1, F)
    hipmod.debug_punctual_sample_host(lts, 0.5, hits, l1)
    for bad, q in ((with_(1, "type", 3), 0.5), (with_(2, "direction", (0.0, 0.0, 0.0)), 0.5), (lts, 0.0), (lts, 1.5), (lts, np.nan)):
        with pytest.raises(hipmod.RptError):
            hipmod.debug_punctual_sample_host(bad, q, hits, l1)


# ---- the restatement's segment mode, ray by ray ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    so = tmp_path_factory.mktemp("lights_segment") / "libanyhit_sim.so"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-msse4.1", "-pthread", "-shared", "-o", str(so),
                    os.path.join(root, "tools", "anyhit_order_sim.cpp")], check=True)
    return C.CDLL(str(so))


@pytest.mark.parametrize("name", ["room", "textured"])
def test_the_restatements_segment_walk_is_the_order_simulators(sim, oracle, name):
    """tests/lights_oracle shadow_ray_hits against tools/anyhit_order_sim.cpp: mode 1 == sim_any_hit_segment (the reference's near-first order and a
    pseudo-random one: `.hit` does not depend on the order), mode 0 == the reference's walk — on rays that end on and around geometry, and on the shadow rays
    the scene's point and spot lights receive from points of its surfaces (max_t = d - 2 EPS from hit + L EPS, as the rule has them)"""
    from test_anyhit_order import _shadow_like_rays
    w = model_scenes.scene(name)[0]
    sc = oracle.scene(w, skybox_f32=model_scenes.scene(name)[2])
    rng = np.random.default_rng(5)
    o, d, max_t = _shadow_like_rays(rng, 20000, w)
    v = w.per_vertex["vertex"][:, :3]
    tri = w.indices[rng.integers(0, len(w.indices), 6000)]
    b = rng.dirichlet((1.0, 1.0, 1.0), 6000).astype(F)
    hit = (b[:, :1] * v[tri["v0"]] + b[:, 1:2] * v[tri["v1"]] + b[:, 2:] * v[tri["v2"]]).astype(F)
    lts = lights_ref.lights(name)
    pos = lts["position"][rng.integers(0, 2, 6000)]                   # the point and the spot light
    to = (pos - hit).astype(F)
    dist = np.sqrt((to * to).sum(1), dtype=F)
    L = (to / dist[:, None]).astype(F)
    o, d = np.concatenate([o, hit + L * F(0.001)]).astype(F), np.concatenate([d, L]).astype(F)
    max_t = np.concatenate([max_t, dist - F(0.001) * F(2)]).astype(F)
    n = len(max_t)
    want = np.zeros(n, np.uint8)
    for mode, seed in ((0, 0), (4, 12345)):
        assert sim.sim_any_hit_segment(C.byref(sc), C.c_size_t(n), lights_ref._p(o), lights_ref._p(d), lights_ref._p(max_t), C.c_int(mode), C.c_uint32(seed),
                                       lights_ref._p(want)) == 0
        got = lights_ref.shadow_rays(sc, o, d, max_t, 1)
        assert np.array_equal(got, want), int((got != want).sum())
    assert 0 < want.sum() < n and 0 < want[20000:].sum() < 6000
    exact = np.zeros(n, np.uint8)
    assert sim.sim_any_hit_order(C.byref(sc), C.c_size_t(n), lights_ref._p(o), lights_ref._p(d), lights_ref._p(max_t), C.c_int(0), C.c_uint32(0), lights_ref._p(exact)) == 0
    assert np.array_equal(lights_ref.shadow_rays(sc, o, d, max_t, 0), exact)
    assert not (want & ~exact).any()                                  # the segment rule can lose an occlusion, never invent one
    print(name, "occlusions the segment rule loses:", int((exact & ~want).sum()), "of", int(exact.sum()))


@pytest.mark.parametrize("nee", [1, 2])
def test_the_segment_mode_leaves_everything_but_occlusions_alone(oracle, nee):
    """rng, ray counts and elisions of the two modes' restatements are equal; a pixel differs only where a shadow ray's `.hit` does"""
    a, a_rng, a_st = lights_ref.reference(oracle, "room", nee, W, H, 2)
    b, b_rng, b_st = lights_ref.reference(oracle, "room", nee, W, H, 2, shadow_mode=1)
    assert np.array_equal(a_rng, b_rng)
    assert (a_st.extension_rays, a_st.shadow_rays, a_st.sky_evals, a_st.shadow_rays_zero_term, a_st.punctual_picks) == \
           (b_st.extension_rays, b_st.shadow_rays, b_st.sky_evals, b_st.shadow_rays_zero_term, b_st.punctual_picks)
    assert np.all(b[..., :3] >= a[..., :3])                              # a lost occlusion only ever adds light


def test_the_loader_drops_a_light_the_setter_would_refuse(rpt, hipmod, tmp_path):
    """a spot or directional light under a node scaled to zero has no direction; a type that is no string, a colour that is no three numbers, a negative or
    infinite intensity: what the file cannot turn into a record the setter accepts is left out (a colour of the wrong kind is the default), the rest loads"""
    import json
    import struct
    path = _lights_glb(tmp_path / "odd.glb")
    data = open(path, "rb").read()
    jlen = struct.unpack_from("<I", data, 12)[0]
    doc, rest = json.loads(data[20:20 + jlen]), data[20 + jlen:]
    ref = lambda i: {"KHR_lights_punctual": {"light": i}}
    first = len(doc["nodes"])
    flat = {"translation": [4.0, 5.0, 6.0], "scale": [0.0, 0.0, 0.0]}
    doc["nodes"] += [dict(flat, extensions=ref(0)), dict(flat, extensions=ref(1)), dict(flat, extensions=ref(2)),      # spot, directional: dropped; point: kept
                     {"extensions": ref(3)}, {"extensions": ref(4)}, {"extensions": ref(5)}, {"extensions": ref(6)}, {"extensions": ref(99)}]
    doc["nodes"][0]["children"] += list(range(first, first + 8))
    doc["extensions"]["KHR_lights_punctual"]["lights"] += [{"type": 7, "intensity": 1.0},                                # 3: a type that is no string
                                                           {"type": "point", "color": ["a", "b", "c"], "intensity": 2.0},  # 4: kept, with the default colour
                                                           {"type": "point", "intensity": -1.0},                           # 5: negative
                                                           {"type": "point", "intensity": 1e60}]                           # 6: infinite as a float
    js = json.dumps(doc).encode()
    js += b" " * (-len(js) % 4)
    open(path, "wb").write(struct.pack("<III", 0x46546C67, 2, 12 + 8 + len(js) + len(rest)) + struct.pack("<II", len(js), 0x4E4F534A) + js + rest)
    got = rpt.World.from_path(path, punctual_lights=True).punctual_lights
    assert got["type"].tolist() == [1, 2, 0, 0, 0, 0]
    assert got["position"][4].tolist() == [4.0, 6.0, 5.0] and got["intensity"][5].tolist() == [2.0, 2.0, 2.0]
    assert hipmod.debug_punctual_lights_check(got, 0.5, True) == (0, "")      # what the loader hands out, the setter takes
