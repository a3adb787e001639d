"""What the camera-lens tests share (tests/test_camera_lens.py, tests/test_gpu_camera_lens.py): the ctypes face of oracle/liblens_oracle.so (source:
tests/lens_oracle), the cases, references computed once per process, and an independent float64 reading of the formulas of csrc/k_lens.h."""
import ctypes as C
import importlib
import os

import numpy as np

import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32

# LDS_PRIMES[0], [1], [2], [31] (kernels/src/rng.rs:20-32): lens u1, jitter x, jitter y, lens u2
P0, P1, P2, P31 = 0x6A09E667, 0xBB67AE84, 0x3C6EF372, 0x720DCDFC

# tan_half_fov, aperture_radius, focus_distance
LENSES = {
    "fov": (0.6, 0.0, 1.0),
    "aperture": (1.0, 0.05, 2.5),
    "both": (0.45, 0.08, 3.0),
    "narrow": (0.25, 0.0, 1.0),
    "wide": (3.0, 0.02, 1.5),
}


class LensStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("extension_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("sky_evals", C.c_uint64),
                ("light_index_clamped", C.c_uint64), ("shadow_rays_zero_term", C.c_uint64), ("error_flags", C.c_uint32), ("threads", C.c_uint32)]


_lib = None


def lens_lib():
    global _lib
    if _lib is None:
        path = os.path.join(os.path.dirname(HERE), "oracle", "liblens_oracle.so")      # beside liboracle.so: build products stay out of tests/
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make lens_oracle`")
        _lib = C.CDLL(path)
    return _lib


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def hipmod():
    return importlib.import_module("rust-path-tracer_amd.hip")


def lens(name_or_fields):
    """a CameraLens of a case name, of (tan_half_fov, aperture_radius, focus_distance), or None for None"""
    if name_or_fields is None:
        return None
    fields = LENSES[name_or_fields] if isinstance(name_or_fields, str) else name_or_fields
    return hipmod().camera_lens(*fields)


def lens_trace_cpu(config, oracle_scene, lens_record, rng, n_samples, rect=None, threads=0):
    """-> (accum (H, W, 4) float32 sums, rng after, LensStats); lens_record: a CameraLens or None (the default record)"""
    W, H = config.width, config.height
    rng = np.ascontiguousarray(rng).copy()
    accum = np.zeros((H, W, 4), F)
    r = np.array(rect if rect else (0, 0, W, H), np.uint32)
    st = LensStats()
    rc = lens_lib().lens_trace_cpu(C.byref(config), C.byref(oracle_scene), None if lens_record is None else C.byref(lens_record), _p(rng), _p(accum),
                                   C.c_uint32(n_samples), _p(r), C.c_int(threads), C.byref(st))
    assert rc == 0 and st.error_flags == 0, (rc, st.error_flags)
    return accum, rng, st


def lens_rays(config, lens_record, pixels_xy, keys):
    """the restatement's camera rays of (x | y << 16, key) pairs: (origins, dirs), (n, 3) float32 each"""
    pixels_xy, keys = np.ascontiguousarray(pixels_xy, np.uint32), np.ascontiguousarray(keys, np.uint32)
    o, d = np.zeros((len(keys), 3), F), np.zeros((len(keys), 3), F)
    rc = lens_lib().lens_rays(C.byref(config), None if lens_record is None else C.byref(lens_record), _p(pixels_xy), _p(keys), C.c_size_t(len(keys)), _p(o), _p(d))
    assert rc == 0
    return o, d


def pairs(width, height, n=4096, seed=5):
    """n (pixel, key) pairs: the image's corners and centre among them, keys over the whole 32-bit range with 0 and 2^32 - 1"""
    g = np.random.default_rng(seed)
    x, y = g.integers(0, width, n), g.integers(0, height, n)
    x[:5], y[:5] = (0, width - 1, 0, width - 1, width // 2), (0, 0, height - 1, height - 1, height // 2)
    keys = g.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys[:2] = (0, 0xFFFFFFFF)
    return (x | (y << 16)).astype(np.uint32), keys


# ---- the scenes and cameras of the image comparisons ------------------------------------------------------------------------------------------------------
def scene_and_view(world, which):
    """(world, skybox, configuration overrides) of "DarkCornell" (its default camera) and "textured" (tests/scenes.py, an image sky)"""
    if which == "DarkCornell":
        return world("DarkCornell"), None, {}
    w, skybox = scenes.textured_scene()
    return w, skybox, dict(has_skybox=1, cam_position=(0.0, 1.8, -1.8, 0.0), cam_rotation=(0.15, 0.0, 0.0, 0.0))


def config(world, which, nee, width, height, **more):
    rpt = importlib.import_module("rust-path-tracer_amd")
    _, _, view = scene_and_view(world, which)
    return rpt.default_config(width, height, nee=nee, **dict(view, **more))


_references = {}


def reference(oracle, world, which, nee, lens_name, width, height, spp):
    """the restatement's accumulator, rng and counters, computed once per process, shared and read-only"""
    key = (which, nee, lens_name, width, height, spp)
    if key not in _references:
        rpt = importlib.import_module("rust-path-tracer_amd")
        w, skybox, _ = scene_and_view(world, which)
        acc, rng, st = lens_trace_cpu(config(world, which, nee, width, height), oracle.scene(w, skybox_f32=skybox), lens(lens_name), rpt.blue_noise_seeds(width, height), spp)
        acc.setflags(write=False)
        rng.setflags(write=False)
        _references[key] = (acc, rng, st)
    return _references[key]


_samples = {}


def per_sample_radiances(oracle, world, which, nee, lens_name, width, height, spp):
    """every sample's radiance, (spp, H, W, 3): one-sample calls of the restatement chained through the returned rng (tests/moments_ref.py SampleBank)"""
    key = (which, nee, lens_name, width, height, spp)
    if key not in _samples:
        rpt = importlib.import_module("rust-path-tracer_amd")
        w, skybox, _ = scene_and_view(world, which)
        cfg, sc, rng = config(world, which, nee, width, height), oracle.scene(w, skybox_f32=skybox), rpt.blue_noise_seeds(width, height)
        out = []
        for _ in range(spp):
            acc, rng, _st = lens_trace_cpu(cfg, sc, lens(lens_name), rng, 1)
            out.append(acc[..., :3].copy())
        _samples[key] = np.stack(out)
        _samples[key].setflags(write=False)
    return _samples[key]


def centre_rays(cfg, tan_half, oracle):
    """the rays of the denoiser's guides under a lens — through the pixel centre and the LENS CENTRE, csrc/k_lens.h lens_ray_centre — in the form of
    tests/denoise_ref.py camera_rays, which they are bit for bit at tan_half 1.0 (tests/test_camera_lens.py): that function with the film scaled"""
    import denoise_ref
    w, h = cfg.width, cfg.height
    ys, xs = np.mgrid[0:h, 0:w]
    sx, sy = xs.astype(F) + F(0.5), ys.astype(F) + F(0.5)
    ux = (sx / F(w)) * F(2.0) - F(1.0)
    uy = (F(1.0) - sy / F(h)) * F(2.0) - F(1.0)
    uy = uy * (F(h) / F(w))
    ux, uy = ux * F(tan_half), uy * F(tan_half)
    v = np.stack([ux, uy, np.ones_like(ux)], -1).astype(F)
    v = v * (F(1.0) / np.sqrt(denoise_ref.dot3(v, v)))[..., None]
    sin = lambda a: oracle.math(0, np.array([a], F))[0]
    cos = lambda a: oracle.math(1, np.array([a], F))[0]
    sy_, cy_ = sin(cfg.cam_rotation[1]), cos(cfg.cam_rotation[1])
    sx_, cx_ = sin(cfg.cam_rotation[0]), cos(cfg.cam_rotation[0])
    z, o = F(0.0), F(1.0)
    ry = np.array([[cy_, z, -sy_], [z, o, z], [sy_, z, cy_]], F)          # columns (Mat3::from_rotation_y)
    rx = np.array([[o, z, z], [z, cx_, sx_], [z, -sx_, cx_]], F)
    m = np.zeros((3, 3), F)                                                # columns of ry * rx
    for c in range(3):
        for r in range(3):
            acc = F(ry[0][r] * rx[c][0])
            acc = F(acc + F(ry[1][r] * rx[c][1]))
            acc = F(acc + F(ry[2][r] * rx[c][2]))
            m[c][r] = acc
    d = m[0][None, None, :] * v[..., 0:1]
    d = d + m[1][None, None, :] * v[..., 1:2]
    d = d + m[2][None, None, :] * v[..., 2:3]
    o3 = np.broadcast_to(np.array(list(cfg.cam_position)[:3], F), d.shape)
    return np.ascontiguousarray(o3.reshape(-1, 3), F), np.ascontiguousarray(d.reshape(-1, 3), F)


# ---- float64 ---------------------------------------------------------------------------------------------------------------------------------------------
def rays_f64(config, fields, pixels_xy, keys):
    """csrc/k_lens.h's formulas read in float64 from their mathematical statement — the only f32 values are the inputs (the record, the configuration and
    the four LDS draws, which ARE f32 numbers): (origins, dirs, focus points in world space, lens offsets (lx, ly) in camera space)"""
    tan_half, aperture, focus = (float(F(v)) for v in fields)
    W, H = float(config.width), float(config.height)
    px, py = (pixels_xy & 0xFFFF).astype(np.float64), (pixels_xy >> 16).astype(np.float64)
    key = keys.astype(np.uint64)

    def unit(prime):
        return ((key * np.uint64(prime)) & np.uint64(0xFFFFFFFF)).astype(F).astype(np.float64) * 2.0 ** -32      # (f32)(v) * 2^-32: the draw is this f32 number

    j1, j2, u1, u2 = unit(P1), unit(P2), unit(P0), unit(P31)
    ux = ((px + j1) / W * 2.0 - 1.0) * tan_half
    uy = ((1.0 - (py + j2) / H) * 2.0 - 1.0) * (H / W) * tan_half
    d = np.stack([ux, uy, np.ones_like(ux)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    pitch, yaw = float(config.cam_rotation[0]), float(config.cam_rotation[1])
    cy, sy, cx, sx = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    rot_y = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])           # Mat3::from_rotation_y
    rot_x = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])           # Mat3::from_rotation_x
    E = rot_y @ rot_x
    cam = np.array([float(config.cam_position[i]) for i in range(3)])
    r = aperture * np.sqrt(u1)
    phi = 2.0 * np.pi * u2
    l = np.stack([r * np.cos(phi), r * np.sin(phi), np.zeros_like(r)], -1)
    pf = d * (focus / d[:, 2:3])
    if aperture == 0.0:
        l = np.zeros_like(l)
    ro = cam + l @ E.T
    rd = pf - l
    rd /= np.linalg.norm(rd, axis=-1, keepdims=True)
    return ro, rd @ E.T, cam + pf @ E.T, l[:, :2]
