"""The thin-lens camera (rpt_set_camera_lens; csrc/k_lens.h) without a GPU: the restatement tests/lens_oracle against the oracle under the default record, the host
build of the header (rpt_debug_lens_rays_host) against the restatement's rays bit for bit, both against an independent float64 reading of the formulas,
and the refusals of the record itself (the context's refusals need a device: tests/test_gpu_camera_lens.py)."""
import numpy as np
import pytest

import lens_ref
from lens_ref import F, LENSES

W, H, SPP = 40, 36, 4
CAMERAS = [dict(cam_position=(0.3, 1.1, -2.4, 0.0), cam_rotation=(0.21, -0.47, 0.0, 0.0)),
           dict(cam_position=(-120.5, 33.0, 410.25, 0.0), cam_rotation=(-0.9, 2.6, 0.0, 0.0))]
PAIRS_W, PAIRS_H = 333, 187         # the image of the ray comparisons: odd, not square

# The largest relative deviation of the host hook from float64 over the 4 096 pairs x 5 lenses x 2 cameras below — the largest of |rd - rd64| (unit vectors),
# |ro - ro64| / |ro64| and (distance of the f64 focus point from the f32 ray) / (its distance from the origin) — measured with
#   python -m pytest tests/test_camera_lens.py -k float64 -s
# which prints it; the tolerance is eight times that (the rule of tests/f64_probes.py).  DESIGN.md 7 N15 quotes the figure.
LENS_REL_MAX = 9.714e-6     # (the far camera, |cam_position| = 430, a focus plane 1.5 away: the origin rounds at 3e-5; at the near camera 4.1e-7)
LENS_TOL = 8 * LENS_REL_MAX


def same_words(a, b):
    return np.array_equal(np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32))


@pytest.mark.parametrize("nee", [0, 1])       # none, MIS
@pytest.mark.parametrize("which", ["DarkCornell", "textured"])
@pytest.mark.parametrize("record", [None, (1.0, 0.0, 1.0), (1.0, 0.0, 7.5)])
def test_default_record_is_the_oracle_word_for_word(oracle, rpt, world, which, nee, record):
    """accumulators, rng and counters of lens_trace_cpu == oracle_trace_cpu: no record, the default one, and an inactive one with another focus"""
    w, skybox, _ = lens_ref.scene_and_view(world, which)
    cfg, sc, seeds = lens_ref.config(world, which, nee, W, H), oracle.scene(w, skybox_f32=skybox), rpt.blue_noise_seeds(W, H)
    acc, rng, st = lens_ref.lens_trace_cpu(cfg, sc, lens_ref.lens(record), seeds, SPP)
    want_acc, want_rng, want = oracle.trace_cpu(cfg, sc, seeds, SPP)
    assert same_words(acc, want_acc) and np.array_equal(rng, want_rng)
    assert (st.samples, st.extension_rays, st.shadow_rays, st.sky_evals, st.light_index_clamped) == \
           (want.samples, want.extension_rays, want.shadow_rays, want.sky_evals, want.light_index_clamped)
    dead = oracle.dead_shadow_rays(cfg, sc, seeds, SPP)
    assert (st.shadow_rays, st.shadow_rays_zero_term) == dead[:2]


@pytest.mark.parametrize("camera", [0, 1])
@pytest.mark.parametrize("name", sorted(LENSES))
def test_host_hook_is_the_restatement_bit_for_bit(hipmod, rpt, name, camera):
    cfg = rpt.default_config(PAIRS_W, PAIRS_H, **CAMERAS[camera])
    xy, keys = lens_ref.pairs(PAIRS_W, PAIRS_H)
    o, d = hipmod.lens_rays_host(cfg, lens_ref.lens(name), xy, keys)
    want_o, want_d = lens_ref.lens_rays(cfg, lens_ref.lens(name), xy, keys)
    assert same_words(o, want_o) and same_words(d, want_d)
    if LENSES[name][1] == 0.0:
        assert same_words(o, np.broadcast_to(np.array(CAMERAS[camera]["cam_position"][:3], F), o.shape))      # a pinhole: every ray leaves cam_position


def test_default_record_gives_the_reference_camera(hipmod, rpt, oracle):
    """NULL and {1, 0, *}: the host hook == the restatement == the rays the oracle's trace_pixel starts with (its first hit distances agree where it dumps them
    is not needed: the restatement under the default record IS checked against the oracle's images above)"""
    cfg = rpt.default_config(PAIRS_W, PAIRS_H, **CAMERAS[0])
    xy, keys = lens_ref.pairs(PAIRS_W, PAIRS_H)
    base = hipmod.lens_rays_host(cfg, None, xy, keys)
    for record in ((1.0, 0.0, 1.0), (1.0, 0.0, 123.0)):
        got = hipmod.lens_rays_host(cfg, lens_ref.lens(record), xy, keys)
        assert same_words(got[0], base[0]) and same_words(got[1], base[1])
    want = lens_ref.lens_rays(cfg, None, xy, keys)
    assert same_words(base[0], want[0]) and same_words(base[1], want[1])


def deviations(hipmod, rpt, name, camera):
    """the host hook against float64 for one lens and camera: the three relative deviations and what the property checks need"""
    cfg = rpt.default_config(PAIRS_W, PAIRS_H, **CAMERAS[camera])
    xy, keys = lens_ref.pairs(PAIRS_W, PAIRS_H)
    o, d = (a.astype(np.float64) for a in hipmod.lens_rays_host(cfg, lens_ref.lens(name), xy, keys))
    ro, rd, focus, l = lens_ref.rays_f64(cfg, LENSES[name], xy, keys)
    to_focus = focus - o
    along = np.sum(to_focus * d, -1, keepdims=True)
    miss = np.linalg.norm(to_focus - along * d, axis=-1) / np.linalg.norm(to_focus, axis=-1)
    return dict(o=o, d=d, ro=ro, cfg=cfg, dir=np.linalg.norm(d - rd, axis=-1).max(), origin=(np.linalg.norm(o - ro, axis=-1) / np.linalg.norm(ro, axis=-1)).max(),
                focus=miss.max(), l=l)


def test_float64_reading_of_the_formulas(hipmod, rpt):
    """every f32 ray is unit length, passes the float64 focus point and leaves the lens disk; origin and direction are float64's within LENS_TOL"""
    worst = 0.0
    for camera in (0, 1):
        for name in sorted(LENSES):
            v = deviations(hipmod, rpt, name, camera)
            worst = max(worst, v["dir"], v["origin"], v["focus"])
            print(f"camera {camera} lens {name:9s} direction {v['dir']:.3e} origin {v['origin']:.3e} focus miss {v['focus']:.3e}")
    print(f"largest relative deviation of the host hook from float64: {worst:.3e} (LENS_REL_MAX {LENS_REL_MAX:.3e})")
    for camera in (0, 1):
        for name in sorted(LENSES):
            v = deviations(hipmod, rpt, name, camera)
            assert v["dir"] <= LENS_TOL and v["origin"] <= LENS_TOL and v["focus"] <= LENS_TOL, (camera, name, v["dir"], v["origin"], v["focus"])
            assert np.abs(np.linalg.norm(v["d"], axis=-1) - 1.0).max() <= LENS_TOL
            # on the lens disk: in the plane through cam_position spanned by the camera's x and y axes, within the radius
            cfg, aperture = v["cfg"], float(F(LENSES[name][1]))
            cam = np.array([cfg.cam_position[i] for i in range(3)], np.float64)
            pitch, yaw = float(cfg.cam_rotation[0]), float(cfg.cam_rotation[1])
            forward = np.array([np.sin(yaw) * np.cos(pitch), -np.sin(pitch), np.cos(yaw) * np.cos(pitch)])      # RotY(yaw) RotX(pitch) (0, 0, 1)
            off = v["o"] - cam
            scale = np.linalg.norm(v["ro"], axis=-1)
            assert (np.abs(off @ forward) <= LENS_TOL * scale).all()
            assert (np.linalg.norm(off, axis=-1) <= aperture + LENS_TOL * scale).all()
            if aperture > 0.0:
                assert np.linalg.norm(off, axis=-1).max() > 0.9 * aperture       # ... and they do spread over it
                assert np.allclose(np.linalg.norm(v["l"], axis=-1), np.linalg.norm(off, axis=-1), atol=float(LENS_TOL * scale.max()))


def test_the_host_hook_refuses_what_the_setter_refuses(hipmod, rpt):
    cfg = rpt.default_config(PAIRS_W, PAIRS_H)
    xy, keys = lens_ref.pairs(PAIRS_W, PAIRS_H, n=8)
    cases = {"tan_half_fov": [(0.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (np.inf, 0.0, 1.0), (np.nan, 0.0, 1.0)],
             "aperture_radius": [(1.0, -0.1, 1.0), (1.0, np.inf, 1.0), (1.0, np.nan, 1.0)],
             "focus_distance": [(1.0, 0.1, 0.0), (1.0, 0.1, -2.0), (1.0, 0.1, np.inf), (1.0, 0.1, np.nan)]}
    for reason, records in cases.items():
        for record in records:
            with pytest.raises(hipmod.RptError) as e:
                hipmod.lens_rays_host(cfg, lens_ref.lens(record), xy, keys)
            assert e.value.code == -1 and reason in str(e.value), (record, str(e.value))
    bad = lens_ref.lens((1.0, 0.0, 1.0))
    bad.reserved = 1
    with pytest.raises(hipmod.RptError) as e:
        hipmod.lens_rays_host(cfg, bad, xy, keys)
    assert e.value.code == -1 and "reserved" in str(e.value)
    for record in ((1.0, 0.0, 0.0), (1.0, 0.0, np.nan), (2.0, 0.0, -1.0)):       # the focus is read only with an aperture
        hipmod.lens_rays_host(cfg, lens_ref.lens(record), xy, keys)


def test_restated_centre_rays_are_denoise_refs_at_the_reference_camera(rpt, oracle):
    """lens_ref.centre_rays, which the GPU tests feed to the guide restatement of tests/denoise_ref.py, is that file's camera_rays at tan_half_fov 1 bit for bit;
    under a field of view its rays are the host hook's film direction within an f32 rounding or two (both normalise the same scaled film point)"""
    import denoise_ref
    cfg = rpt.default_config(W, H, **CAMERAS[0])
    plain, ours = denoise_ref.camera_rays(cfg, oracle), lens_ref.centre_rays(cfg, 1.0, oracle)
    assert same_words(plain[0], ours[0]) and same_words(plain[1], ours[1])
    scaled = lens_ref.centre_rays(cfg, 0.6, oracle)
    assert same_words(scaled[0], plain[0]) and not same_words(scaled[1], plain[1])
    centre = scaled[1].reshape(H, W, 3)[H // 2, W // 2].astype(np.float64), plain[1].reshape(H, W, 3)[H // 2, W // 2].astype(np.float64)
    corner = scaled[1].reshape(H, W, 3)[0, 0].astype(np.float64), plain[1].reshape(H, W, 3)[0, 0].astype(np.float64)
    assert np.dot(*corner) < 1.0 and np.dot(corner[0], centre[0]) > np.dot(corner[1], centre[1])      # a narrower field of view: the corner ray is closer to the axis


def test_python_helpers(hipmod):
    assert hipmod.tan_half_fov(90) == 1.0 and abs(hipmod.tan_half_fov(60) - 3 ** -0.5) < 1e-12
    d = hipmod.CameraLens()
    hipmod.lib().rpt_camera_lens_default(__import__("ctypes").byref(d))
    assert (d.tan_half_fov, d.aperture_radius, d.focus_distance, d.reserved) == (1.0, 0.0, 1.0, 0)
