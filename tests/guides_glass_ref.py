"""numpy restatement, in f32 and in the same operation order, of the guides that follow glass (include/rpt/rpt.h rpt_set_guides_through_glass,
csrc/k_guides_glass.h): one step of a pixel's chain, and the driver that runs whole chains round by round.

Not a test module (no test_ prefix): tests/test_guides_glass.py holds the host build of the step (hip.glass_step_host) against `step`, and
tests/test_gpu_guides_glass.py the device against the chain.  The walk is the oracle's nearest hit (oracle.trace_rays(scene, 0, ...)), the atlas lookups the
oracle's sampler (oracle.sample_image), the camera rays denoise_ref.camera_rays unless the caller hands in others; everything else is plain IEEE f32 arithmetic, which numpy performs
operation by operation without fusing.  `run_chains` takes the step as a function, so the same rounds drive the restatement and the host build.
"""
import numpy as np

from denoise_ref import camera_rays, dot3, finite3

F = np.float32
KIND_MISS, KIND_SURFACE, KIND_EMITTER = 0, 1, 2
MODEL_GLASS = 2
EPS = F(0.001)                 # util.rs:5
MISS_LENGTH = F(1e6)


def normalize(v):
    """Vec3::normalize = v * (1 / length)"""
    return (v * (F(1.0) / np.sqrt(dot3(v, v)))[..., None]).astype(F)


def fmax0(x):
    """f32::max(x, 0): a NaN yields 0"""
    return np.where(x > F(0.0), x, F(0.0)).astype(F)


def shade_hits(world, oracle, ro, rd, t, tri):
    """every ray's hit shaded as the first-hit guide shades it (csrc/k_denoise.h k_dn_shade_guides): (emits, normal, a, material index); rows of rays that
    missed hold the values of triangle `tri` all the same and are not to be read"""
    hit_point = (ro + rd * t[:, None]).astype(F)
    idx = world.indices[tri]
    mi = idx["material"]
    mat = world.materials[mi]
    emits = (mat["emissive"][:, :3] != 0).any(axis=1)
    pa, pb, pc = (world.per_vertex[idx[k]] for k in ("v0", "v1", "v2"))
    a3 = pa["vertex"][:, :3]
    v0, v1, v2 = pb["vertex"][:, :3] - a3, pc["vertex"][:, :3] - a3, hit_point - a3
    d00, d01, d11, d20, d21 = dot3(v0, v0), dot3(v0, v1), dot3(v1, v1), dot3(v2, v0), dot3(v2, v1)
    denom = d00 * d11 - d01 * d01
    bv = (d11 * d20 - d01 * d21) / denom
    bw = (d00 * d21 - d01 * d20) / denom
    bu = F(1.0) - bv - bw
    interp = lambda f, k: (bu[:, None] * pa[f][:, :k] + bv[:, None] * pb[f][:, :k] + bw[:, None] * pc[f][:, :k]).astype(F)
    nrm = interp("normal", 3)
    a = np.where(emits[:, None], F(1.0), mat["albedo"][:, :3]).astype(F)
    atlas = getattr(world, "atlas", None)
    textured = bool(np.any([world.materials[k] != 0 for k in ("has_albedo_texture", "has_metallic_texture", "has_roughness_texture", "has_normal_texture")]))
    if textured:
        uv = ((bu[:, None] * pa["uv0"] + bv[:, None] * pb["uv0"]) + bw[:, None] * pc["uv0"]).astype(F)
        clamped = np.where(uv > F(0.0), uv, F(0.0))                                   # fminr(fmaxr(uv, 0), 1): a NaN yields the other operand
        clamped = np.where(clamped < F(1.0), clamped, F(1.0))
        wrap = (clamped != uv).any(axis=1)
        uv = np.where(wrap[:, None], uv - np.floor(uv), uv).astype(F)
        has_n = mat["has_normal_texture"] != 0
        if has_n.any():
            r = mat["normals"][has_n]
            s = oracle.sample_image(atlas, np.stack([r[:, 0] + uv[has_n, 0] * r[:, 2], r[:, 1] + uv[has_n, 1] * r[:, 3]], -1).astype(F))[:, :3]
            nm = (s * F(2.0) - F(1.0)).astype(F)
            n0 = nrm[has_n]
            tangent = interp("tangent", 3)[has_n]
            bitangent = np.cross(tangent, n0).astype(F)
            mapped = (tangent * nm[:, 0:1]).astype(F)
            mapped = (mapped + bitangent * nm[:, 1:2]).astype(F)
            mapped = (mapped + n0 * nm[:, 2:3]).astype(F)
            nrm[has_n] = normalize(mapped)                                            # lib.rs:141; the guide normalises once more below
        has_a = (mat["has_albedo_texture"] != 0) & ~emits
        if has_a.any():
            r = mat["albedo"][has_a]
            a[has_a] = oracle.sample_image(atlas, np.stack([r[:, 0] + uv[has_a, 0] * r[:, 2], r[:, 1] + uv[has_a, 1] * r[:, 3]], -1).astype(F))[:, :3]
    nrm = normalize(nrm)
    nrm = np.where(finite3(nrm)[:, None], nrm, F(0.0)).astype(F)
    return emits, nrm, a, mi, hit_point


def step(world, models, K, oracle, ro, rd, t, tri, flags, A, L, m):
    """One step of every ray's chain (include/rpt/rpt.h "guides that follow glass"): the rays (n, 3), their nearest hits, the chains so far (A (n, 3), L, m).
    -> what hip.glass_step_host returns."""
    ro, rd, A = (np.array(x, F).reshape(-1, 3) for x in (ro, rd, A))
    t, L, m = np.asarray(t, F), np.array(L, F), np.array(m, np.uint32)
    n = len(ro)
    hit = (np.asarray(flags) & 1) != 0
    tri = np.where(hit, tri, 0)
    with np.errstate(all="ignore"):
        emits, nrm, a, mi, hit_point = shade_hits(world, oracle, ro, rd, t, tri)
        Aa = (A * a).astype(F)
        # a miss: kind 0, normal 0, albedo A, L += 1e6.  A hit: L += t (the origin's dir * EPS shifts are not part of L)
        L_out = np.where(hit, L + t, L + MISS_LENGTH).astype(F)
        kind = np.where(hit, np.where(emits, KIND_EMITTER, KIND_SURFACE), KIND_MISS).astype(np.uint32)
        normal = np.where(hit[:, None], nrm, F(0.0)).astype(F)
        albedo = np.where(hit[:, None], Aa, A).astype(F)
        glass = hit & ~emits & ((models["model"][mi] == MODEL_GLASS) if models is not None else np.zeros(n, bool))
        zero_normal = (nrm == 0).all(axis=1)
        wants_on = glass & (m < K) & ~zero_normal
        ior = (models["ior"][mi] if models is not None else np.ones(n, F)).astype(F)
        # Glass::sample at zero roughness (bsdf.rs:128-165), the microsurface normal = the guide's normal
        view = (-rd).astype(F)
        inside = dot3(nrm, view) < 0
        npr = np.where(inside[:, None], -nrm, nrm).astype(F)
        in_ior, out_ior = np.where(inside, ior, F(1.0)).astype(F), np.where(inside, F(1.0), ior).astype(F)
        c = dot3(view, npr)
        f0 = (in_ior - out_ior) / (in_ior + out_ior)
        f0 = f0 * f0
        x = F(1.0) - fmax0(c)
        x2 = x * x
        x4 = x2 * x2
        fresnel = f0 + (F(1.0) - f0) * (x * x4)                                        # fresnel_schlick_scalar, util.rs:233-236: powi(5) = x * ((x x) (x x))
        reflect = fresnel > F(0.5)
        dir_reflect = normalize((F(2.0) * np.abs(c))[:, None] * npr - view)
        eta = in_ior / out_ior
        # f32::signum: the sign bit decides, so signum(+0.0) = +1 and signum(-0.0) = -1 (c == 0 made explicit); a NaN stays a NaN
        sg = np.where(c == 0, np.where(np.signbit(c), F(-1.0), F(1.0)), np.where(np.isnan(c), c, np.where(c < 0, F(-1.0), F(1.0)))).astype(F)
        root = np.sqrt(fmax0(F(1.0) + eta * (c * c - F(1.0))))
        dir_refract = normalize((eta * c - sg * root)[:, None] * npr - eta[:, None] * view)
        direction = np.where(reflect[:, None], dir_reflect, dir_refract).astype(F)
        active = wants_on & finite3(direction)
        exhausted = glass & ~active
        kind = np.where(glass, KIND_SURFACE, kind).astype(np.uint32)
        A_out = np.where((active & ~reflect)[:, None], Aa, A).astype(F)
        ro_out = np.where(active[:, None], hit_point + direction * EPS, ro).astype(F)  # lib.rs:172
        rd_out = np.where(active[:, None], direction, rd).astype(F)
        m_out = np.where(active, m + 1, m).astype(np.uint32)
    return {"origins": ro_out, "dirs": rd_out, "albedo_product": A_out, "length": L_out, "interfaces": m_out, "active": active, "kind": kind, "normal": normal,
            "albedo": albedo, "exhausted": exhausted}


def run_chains(step_fn, walk_fn, ro0, rd0, K):
    """Whole chains, round by round, the rays still inside glass kept in ascending order: step_fn(ro, rd, t, tri, flags, A, L, m) -> the dictionary of `step`,
    walk_fn(ro, rd) -> (t, tri, flags).  -> (planes by ray: albedo, normal, position (n, 3), depth, kind (n); info: rounds, rays per round, pixels_through_glass,
    pixels_exhausted); the planes carry "interfaces", the m of every chain, too"""
    ro0, rd0 = np.ascontiguousarray(ro0, F).reshape(-1, 3), np.ascontiguousarray(rd0, F).reshape(-1, 3)
    n = len(ro0)
    out = {"albedo": np.zeros((n, 3), F), "normal": np.zeros((n, 3), F), "depth": np.zeros(n, F), "kind": np.zeros(n, np.uint32),
           "interfaces": np.zeros(n, np.uint32)}
    info = {"rounds": 0, "rays": [0] * 9, "pixels_through_glass": 0, "pixels_exhausted": 0}
    idx = np.arange(n)
    ro, rd, A, L, m = ro0.copy(), rd0.copy(), np.ones((n, 3), F), np.zeros(n, F), np.zeros(n, np.uint32)
    for r in range(K + 1):
        if len(idx) == 0:
            break
        info["rays"][r] = len(idx)
        info["rounds"] = r + 1
        t, tri, flags = walk_fn(ro, rd)
        s = step_fn(ro, rd, t, tri, flags, A, L, m)
        done = ~s["active"]
        at = idx[done]
        out["albedo"][at], out["normal"][at], out["depth"][at], out["kind"][at] = s["albedo"][done], s["normal"][done], s["length"][done], s["kind"][done]
        out["interfaces"][at] = s["interfaces"][done]
        info["pixels_through_glass"] += int((s["interfaces"][done] > 0).sum())
        info["pixels_exhausted"] += int(s["exhausted"][done].sum())
        keep = s["active"]
        idx, ro, rd, A, L, m = idx[keep], s["origins"][keep], s["dirs"][keep], s["albedo_product"][keep], s["length"][keep], s["interfaces"][keep]
    assert len(idx) == 0, "a ray of round K has crossed K interfaces: that round ends every chain"
    with np.errstate(all="ignore"):
        out["position"] = (ro0 + rd0 * out["depth"][:, None]).astype(F)      # unfolded along the primary ray
    return out, info


def image(planes, w, h):
    """the planes by row-major pixel in the layout of Renderer.guides()"""
    return {"albedo": planes["albedo"].reshape(h, w, 3), "normal": planes["normal"].reshape(h, w, 3), "position": planes["position"].reshape(h, w, 3),
            "depth": planes["depth"].reshape(h, w).copy(), "kind": planes["kind"].reshape(h, w), "interfaces": planes["interfaces"].reshape(h, w)}


def oracle_walk(oracle, scene):
    def walk(ro, rd):
        t, tri, flags, _ = oracle.trace_rays(scene, 0, ro, rd)
        return t, tri, flags
    return walk


def guides(world, models, K, cfg, oracle, scene=None, step_fn=None, rays=None):
    """(the guides of rpt_set_guides_through_glass(K) in the layout of Renderer.guides(), the counts of rpt_guides_info_get); step_fn: another build of the
    step with `step`'s signature after (world, models, K, oracle); rays: the primary rays (origins, dirs) by row-major pixel when they are not the reference
    camera's — under a camera lens the rays through the lens centre, tests/lens_ref.py centre_rays"""
    scene = scene if scene is not None else oracle.scene(world)
    ro, rd = rays if rays is not None else camera_rays(cfg, oracle)
    fn = step_fn or (lambda *a: step(world, models, K, oracle, *a))
    planes, info = run_chains(fn, oracle_walk(oracle, scene), ro, rd, K)
    return image(planes, cfg.width, cfg.height), info
