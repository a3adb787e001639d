"""Procedural scenes with material models (include/rpt/rpt.h rpt_set_material_models), built with the host builders as tests/scenes.py builds its own; and the
ctypes face of the bit-exact restatement oracle/libmodels_oracle.so (source: tests/models_oracle).  Every scene function returns (world, records, skybox or None, view):
records as hip.MATERIAL_MODEL_DTYPE, view = the camera fields of a configuration."""
import ctypes as C
import importlib
import os

import numpy as np

import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
MODEL_PBR, MODEL_LAMBERTIAN, MODEL_GLASS = 0, 1, 2
MATERIAL_MODEL_DTYPE = np.dtype([("model", np.uint32), ("ior", np.float32), ("reserved", np.uint32, 2)])

# the largest paths the reference's 31 dimensions allow (rpt_set_config): without NEE 2 + 8 * 3 + 5 roulette draws, with it 2 + 4 * 7 + 1
CONFIGS = {0: dict(nee=0, max_bounces=8, min_bounces=2), 1: dict(nee=1, max_bounces=4, min_bounces=2), 2: dict(nee=2, max_bounces=4, min_bounces=2)}
# A lens with an aperture takes table entry 31 for its own sample (rpt_set_camera_lens refuses a 31-dimension configuration with RPT_ECONFIG), so under one:
# without NEE roulette starts a bounce later, 2 + 8 * 3 + 4 = 30, which keeps eight bounces for the glass; with NEE three bounces and roulette from the third
# on, 2 + 3 * 7 + 1 = 24, which keeps the roulette alive.  A lens without an aperture ("fov", "narrow") leaves the 31 dimensions to the path.
APERTURE_OVERRIDES = {0: dict(min_bounces=3), 1: dict(max_bounces=3, min_bounces=1), 2: dict(max_bounces=3, min_bounces=1)}


def lens_overrides(nee, lens_name):
    """the configuration overrides CONFIGS[nee] needs under the lens of that name (tests/lens_ref.py LENSES; None: no lens)"""
    import lens_ref
    return dict(APERTURE_OVERRIDES[nee]) if lens_name is not None and lens_ref.LENSES[lens_name][1] != 0.0 else {}


def records(models, iors=None):
    rec = np.zeros(len(models), MATERIAL_MODEL_DTYPE)
    rec["model"] = models
    rec["ior"] = 1.5 if iors is None else iors
    return rec


def icosphere(center, radius, subdivisions=2):
    """20 * 4^subdivisions triangles (320 at 2) over shared vertices, so that the vertex normals (position - center, normalised) are smooth; wound outward"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, g = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    n = np.array(v)
    return (np.asarray(center, np.float64) + radius * n).astype(np.float32), n.astype(np.float32), np.array(f, np.uint32)


class _Mesh:
    def __init__(self):
        self.v, self.n, self.t = [], [], []

    def quad(self, corners, normal, material):
        k = len(self.v)
        self.v += [list(map(float, c)) for c in corners]
        self.n += [list(map(float, normal))] * 4
        self.t += [[k, k + 1, k + 2, material], [k, k + 2, k + 3, material]]

    def lamp(self, x0, x1, y, z0, z1, material):
        """facing down: wound so that the geometric normal does too (emitters are single sided)"""
        k = len(self.v)
        self.v += [[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]]
        self.n += [[0.0, -1.0, 0.0]] * 4
        self.t += [[k, k + 2, k + 1, material], [k, k + 3, k + 2, material]]

    def sphere(self, center, radius, material, subdivisions=2):
        p, n, f = icosphere(center, radius, subdivisions)
        k = len(self.v)
        self.v += p.tolist()
        self.n += n.tolist()
        self.t += [[k + int(a), k + int(b), k + int(c), material] for a, b, c in f]

    def world(self, materials):
        """materials: (roughness, metallic, albedo, emissive) each"""
        rpt = importlib.import_module("rust-path-tracer_amd")
        m = np.zeros(len(materials), rpt._ffi.MATERIAL_DTYPE)
        for i, (roughness, metallic, albedo, emissive) in enumerate(materials):
            m["albedo"][i] = list(albedo) + [1.0]
            m["roughness"][i, :] = roughness
            m["metallic"][i, :] = metallic
            m["emissive"][i] = list(emissive) + [1.0 if any(emissive) else 0.0]
        return rpt.World.from_buffers(np.array(self.v, np.float32), np.array(self.n, np.float32), None, np.array(self.t, np.uint32), m)


_BLACK = (0.0, 0.0, 0.0)


def room(subdivisions=2):
    """A closed box with a ceiling lamp: PBR walls (a rough grey one, a metallic one), one wall Lambertian, a glass icosphere of 320 triangles with smooth
    normals (ior 1.5, material roughness 0.05) and a tinted thin pane of two parallel quads."""
    g = _Mesh()
    c = np.array([[-3, 0, -1], [3, 0, -1], [3, 0, 5], [-3, 0, 5], [-3, 4, -1], [3, 4, -1], [3, 4, 5], [-3, 4, 5]], np.float32)
    for q, nrm, mat in (((0, 1, 2, 3), (0, 1, 0), 0), ((7, 6, 5, 4), (0, -1, 0), 0), ((0, 4, 5, 1), (0, 0, 1), 0), ((3, 2, 6, 7), (0, 0, -1), 0),
                        ((0, 3, 7, 4), (1, 0, 0), 1), ((1, 5, 6, 2), (-1, 0, 0), 2)):
        g.quad([c[i] for i in q], nrm, mat)
    g.lamp(-1.0, 1.0, 3.9, 1.0, 3.0, 5)
    g.sphere((0.7, 1.1, 2.4), 0.9, 3, subdivisions)
    g.quad([(-2.4, 0.3, 2.0), (-0.9, 0.3, 2.6), (-0.9, 2.6, 2.6), (-2.4, 2.6, 2.0)], (0.371391, 0.0, -0.928477), 4)          # the pane's front ...
    g.quad([(-2.4186, 0.3, 2.0464), (-0.9186, 0.3, 2.6464), (-0.9186, 2.6, 2.6464), (-2.4186, 2.6, 2.0464)], (-0.371391, 0.0, 0.928477), 4)   # ... and back, 0.05 behind
    w = g.world([(1.0, 0.0, (0.75, 0.75, 0.75), _BLACK), (0.8, 0.0, (0.8, 0.25, 0.2), _BLACK), (0.25, 0.9, (0.3, 0.5, 0.85), _BLACK),
                 (0.05, 0.0, (0.97, 0.98, 1.0), _BLACK), (0.02, 0.0, (0.55, 0.9, 0.65), _BLACK), (1.0, 0.0, _BLACK, (18.0, 17.0, 15.0))])
    rec = records([MODEL_PBR, MODEL_LAMBERTIAN, MODEL_PBR, MODEL_GLASS, MODEL_GLASS, MODEL_PBR], [0.0, 0.0, 0.0, 1.5, 1.45, 0.0])
    return w, rec, None, dict(cam_position=(0.0, 1.6, -0.8, 0.0), cam_rotation=(0.12, 0.0, 0.0, 0.0))


def small_room():
    """The room with an icosphere of 80 triangles: 98 triangles in all, which the device keeps in LDS (rpt_scene.hip: nodes * 50 + triangles * 48 <= 32 KB) —
    the room, the open scene and the furnace, with their 320-triangle spheres, are walked from global memory.  So this is the scene where the models meet
    the LDS walks: the FIRST walk over prepared slots, the LAST walk that ends the paths itself (two emissive triangles)."""
    return room(1)


def open_scene():
    """A glass sphere over a Lambertian ground under the procedural sky: misses, the sky stage, the packed variant's miss binning."""
    g = _Mesh()
    g.quad([(-40, 0, -40), (-40, 0, 40), (40, 0, 40), (40, 0, -40)], (0, 1, 0), 0)
    g.sphere((0.0, 1.0, 3.0), 1.0, 1)
    w = g.world([(0.9, 0.0, (0.7, 0.6, 0.45), _BLACK), (0.05, 0.0, (0.9, 0.95, 1.0), _BLACK)])
    return w, records([MODEL_LAMBERTIAN, MODEL_GLASS]), None, dict(cam_position=(0.0, 1.4, -1.0, 0.0), cam_rotation=(0.1, 0.0, 0.0, 0.0))


def textured():
    """scenes.textured_scene() with the models dealt round-robin over its materials: a texture feeds a Glass or Lambertian albedo (and Glass's roughness),
    a normal map feeds `inside`."""
    w, skybox = scenes.textured_scene()
    n = len(w.materials)
    rec = records([(MODEL_GLASS, MODEL_LAMBERTIAN, MODEL_PBR)[i % 3] for i in range(n)], [1.3 + 0.1 * i for i in range(n)])
    return w, rec, skybox, dict(cam_position=(0.0, 1.8, -1.8, 0.0), cam_rotation=(0.15, 0.0, 0.0, 0.0))


FURNACE_SKY = (0.5, 0.25, 0.75)


def furnace():
    """One glass sphere, albedo (1, 1, 1), alone under a constant image sky."""
    g = _Mesh()
    g.sphere((0.0, 0.0, 3.0), 1.0, 0)
    w = g.world([(0.05, 0.0, (1.0, 1.0, 1.0), _BLACK)])
    sky = np.ones((4, 8, 4), np.float32)
    sky[..., :3] = FURNACE_SKY
    return w, records([MODEL_GLASS]), sky, dict(cam_position=(0.0, 0.0, 0.0, 0.0), cam_rotation=(0.0, 0.0, 0.0, 0.0))


SCENES = {"room": room, "small_room": small_room, "open": open_scene, "textured": textured, "furnace": furnace}
_built = {}


def scene(name):
    """built once per process"""
    if name not in _built:
        _built[name] = SCENES[name]()
    return _built[name]


def config(name, nee, width, height, **more):
    rpt = importlib.import_module("rust-path-tracer_amd")
    _, _, skybox, view = scene(name)
    return rpt.default_config(width, height, has_skybox=0 if skybox is None else 1, **view, **dict(CONFIGS[nee], **more))


# ---- oracle/libmodels_oracle.so (tests/models_oracle) -----------------------------------------------------------------------------------------------------------
class ModelsStats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("extension_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("sky_evals", C.c_uint64),
                ("light_index_clamped", C.c_uint64), ("shadow_rays_zero_term", C.c_uint64), ("error_flags", C.c_uint32), ("threads", C.c_uint32)]


_lib = None


def models_lib():
    global _lib
    if _lib is None:
        path = os.path.join(os.path.dirname(HERE), "oracle", "libmodels_oracle.so")      # beside liboracle.so: build products stay out of tests/
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make models_oracle`")
        _lib = C.CDLL(path)
    return _lib


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def models_trace_cpu(config, oracle_scene, models, rng, n_samples, rect=None, threads=0):
    """-> (accum (H, W, 4) float32 sums, rng after, ModelsStats); models: MATERIAL_MODEL_DTYPE records or None (every material PBR)"""
    W, H = config.width, config.height
    rng = np.ascontiguousarray(rng).copy()
    accum = np.zeros((H, W, 4), np.float32)
    models = None if models is None else np.ascontiguousarray(models, MATERIAL_MODEL_DTYPE)
    r = np.array(rect if rect else (0, 0, W, H), np.uint32)
    st = ModelsStats()
    rc = models_lib().models_trace_cpu(C.byref(config), C.byref(oracle_scene), _p(models), _p(rng), _p(accum), C.c_uint32(n_samples), _p(r), C.c_int(threads),
                                       C.byref(st))
    assert rc == 0 and st.error_flags == 0, (rc, st.error_flags)
    return accum, rng, st


def models_lens_trace_cpu(config, oracle_scene, models, lens_record, rng, n_samples, rect=None, threads=0):
    """models_trace_cpu with the camera of rpt_set_camera_lens: lens_record a CameraLens (tests/lens_ref.py lens), or None for the reference's camera"""
    W, H = config.width, config.height
    rng = np.ascontiguousarray(rng).copy()
    accum = np.zeros((H, W, 4), np.float32)
    models = None if models is None else np.ascontiguousarray(models, MATERIAL_MODEL_DTYPE)
    r = np.array(rect if rect else (0, 0, W, H), np.uint32)
    st = ModelsStats()
    rc = models_lib().models_lens_trace_cpu(C.byref(config), C.byref(oracle_scene), _p(models), None if lens_record is None else C.byref(lens_record), _p(rng),
                                            _p(accum), C.c_uint32(n_samples), _p(r), C.c_int(threads), C.byref(st))
    assert rc == 0 and st.error_flags == 0, (rc, st.error_flags)
    return accum, rng, st


def models_lens_trace_pixel(config, oracle_scene, models, lens_record, x, y, n, offset):
    """one pixel-sample of the restatement -> (its radiance (3,) float32, the error flags)"""
    class Rng(C.Structure):
        _fields_ = [("n", C.c_uint32), ("offset", C.c_uint32)]
    models = None if models is None else np.ascontiguousarray(models, MATERIAL_MODEL_DTYPE)
    out = np.zeros(3, np.float32)
    fn = models_lib().models_lens_trace_pixel
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, Rng, C.c_void_p]
    flags = fn(C.addressof(config), C.addressof(oracle_scene), None if models is None else models.ctypes.data,
               None if lens_record is None else C.addressof(lens_record), x, y, Rng(int(n), int(offset)), out.ctypes.data)
    return out, flags


_references = {}


def reference(oracle, name, nee, width, height, spp, lens=None, records=True, **more):
    """the restatement's accumulator, rng and counters of a scene under CONFIGS[nee] (and `more`), computed once per process and shared; lens: a name of
    tests/lens_ref.py LENSES, or None for the reference's camera; records False: every material PBR"""
    key = (name, nee, width, height, spp, lens, records, tuple(sorted(more.items())))
    if key not in _references:
        import lens_ref
        rpt = importlib.import_module("rust-path-tracer_amd")
        w, rec, skybox, _ = scene(name)
        cfg = config(name, nee, width, height, **more)
        sc, seeds = oracle.scene(w, skybox_f32=skybox), rpt.blue_noise_seeds(width, height)
        if lens is None and records:
            acc, rng, st = models_trace_cpu(cfg, sc, rec, seeds, spp)
        else:
            acc, rng, st = models_lens_trace_cpu(cfg, sc, rec if records else None, lens_ref.lens(lens), seeds, spp)
        acc.setflags(write=False)
        rng.setflags(write=False)
        _references[key] = (acc, rng, st)
    return _references[key]


_samples = {}


def per_sample_radiances(oracle, name, nee, width, height, spp, lens=None, **more):
    """every sample's radiance, (spp, H, W, 3): one-sample calls of the restatement chained through the returned rng (tests/moments_ref.py SampleBank)"""
    key = (name, nee, width, height, spp, lens, tuple(sorted(more.items())))
    if key not in _samples:
        import lens_ref
        rpt = importlib.import_module("rust-path-tracer_amd")
        w, rec, skybox, _ = scene(name)
        cfg, sc, rng = config(name, nee, width, height, **more), oracle.scene(w, skybox_f32=skybox), rpt.blue_noise_seeds(width, height)
        out = []
        for _ in range(spp):
            acc, rng, _st = models_lens_trace_cpu(cfg, sc, rec, lens_ref.lens(lens), rng, 1)
            out.append(acc[..., :3].copy())
        _samples[key] = np.stack(out)
        _samples[key].setflags(write=False)
    return _samples[key]


# ---- the furnace statement (needs no reference) ------------------------------------------------------------------------------------------------------
def furnace_check(acc, s, primary_miss, spp):
    """Under a constant image sky, glass of albedo 1 and no NEE every sample is exactly s — the f32 value a primary miss yields — or exactly 0: Glass has pdf 1
    and spectrum 1 or albedo, and the roulette's prob is 1.  So every pixel is a sequential f32 sum of k <= spp copies of s, k = spp where the primary ray
    misses the sphere.  -> k per pixel"""
    s = np.asarray(s, np.float32)
    sums = np.zeros((spp + 1, 3), np.float32)
    for k in range(1, spp + 1):
        sums[k] = sums[k - 1] + s
    assert np.all(s > 0)
    k = np.full(acc.shape[:2], -1)
    for j in range(spp + 1):
        k[np.all(acc[..., :3].view(np.uint32) == sums[j].view(np.uint32), axis=-1)] = j
    assert np.all(k >= 0), f"{int((k < 0).sum())} pixels are no sum of copies of the sky's value"
    if primary_miss is not None:                            # (None under a lens: the mask below is the reference camera's)
        assert np.all(k[primary_miss] == spp)
    assert np.all(acc[..., 3] == spp)
    return k


def furnace_primary_miss(cfg):
    """pixels whose every jittered primary ray passes the unit sphere at (0, 0, 3) by a margin (camera at the origin, looking down +z)"""
    W, H = cfg.width, cfg.height
    miss = np.ones((H, W), bool)
    for dx in (0.0, 1.0):
        for dy in (0.0, 1.0):
            x, y = np.meshgrid(np.arange(W) + dx, np.arange(H) + dy)
            u = x / W * 2 - 1
            v = ((1 - y / H) * 2 - 1) * H / W
            d = np.stack([u, v, np.ones_like(u)], -1)
            d /= np.linalg.norm(d, axis=-1, keepdims=True)
            b = d[..., 2] * 3.0
            miss &= (9.0 - b * b) > 1.0 + 0.05             # squared distance of the centre from the ray's line against the squared radius
    return miss


def furnace_sky_value(oracle, W, H):
    """s: one sample of a pixel whose primary ray misses"""
    one, _, _ = reference(oracle, "furnace", 0, W, H, 1)
    return one[furnace_primary_miss(config("furnace", 0, W, H))][0, :3].copy()
