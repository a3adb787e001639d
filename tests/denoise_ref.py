"""numpy restatement, in f32 and in the same operation order, of the denoiser of csrc/k_denoise.h: the first-hit guide buffers and the a-trous filter.

Not a test module (no test_ prefix): tests/test_denoise.py and tests/test_gpu_denoise.py hold the library against it.  Two things come from the CPU
oracle instead of numpy, because numpy has no bit-exact counterpart: the exponential (oracle.math(3, .), the rptm::expr the filter calls) and the sine /
cosine of the camera rotation (oracle.math(1 / 0, .)); the nearest hits of the guide rays are oracle.trace_rays(scene, 0, ...), and the display
operators oracle.resolve.  Everything else is plain IEEE f32 arithmetic, which numpy performs operation by operation without fusing.
"""
import numpy as np

F = np.float32
KIND_MISS, KIND_SURFACE, KIND_EMITTER = 0, 1, 2
ALBEDO_FLOOR = F(0.01)
H5 = {-2: F(0.0625), -1: F(0.25), 0: F(0.375), 1: F(0.25), 2: F(0.0625)}


def dot3(a, b):
    """Vec3::dot = (x x' + y y') + z z' over the last axis"""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def finite3(a):
    return np.isfinite(a).all(axis=-1)


def albedo_floor(a):
    """rptm::fmaxr(a, 0.01): a NaN yields the other operand"""
    return np.where(a > ALBEDO_FLOOR, a, ALBEDO_FLOOR).astype(F)


# ---- filter ---------------------------------------------------------------------------------------------------------------------------------------

def filter_pass(e, normal, position, depth, kind, i, normal_power_log2, sigma_color, sigma_plane, expr):
    """dn_filter_pixel for every pixel: pass i (step 2^i) over the (H, W, 3) image e"""
    h, w = e.shape[:2]
    step = 1 << i
    plane_scale = F(F(sigma_plane) * F(step)) * F(F(2.0) / F(w))
    sigma_i = F(F(sigma_color) * F(2.0 ** -i))
    sigma2 = F(sigma_i * sigma_i)
    plane = (plane_scale * depth).astype(F)
    ep2 = dot3(e, e)
    centre_ok = finite3(e)
    total = np.zeros_like(e)
    wsum = np.zeros((h, w), F)
    joined = np.zeros((h, w), bool)
    ys, xs = np.mgrid[0:h, 0:w]
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            k = F(H5[dx] * H5[dy])
            qy, qx = ys + dy * step, xs + dx * step
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
            e_q = e[qy, qx]
            if dx == 0 and dy == 0:
                wt = np.full((h, w), k, F)
                ok = inside
            else:
                ok = inside & (kind[qy, qx] == kind) & finite3(e_q)
                hit = kind != KIND_MISS
                ndot = dot3(normal, normal[qy, qx])
                w_n = np.where(F(0.0) > ndot, F(0.0), np.where(np.isnan(ndot), F(0.0), ndot)).astype(F)      # fmaxr(0, n_p . n_q)
                for _ in range(normal_power_log2):
                    w_n = w_n * w_n
                w_n = np.where(hit, w_n, F(1.0)).astype(F)
                d = np.abs(dot3(normal, position[qy, qx] - position)) / plane
                d = np.where(hit, d, F(0.0)).astype(F)
                if sigma2 != 0.0:
                    diff = e - e_q
                    d = d + dot3(diff, diff) / (sigma2 * ((ep2 + dot3(e_q, e_q)) + F(1e-12)))
                wt = (k * w_n) * expr((-d).astype(F))
                ok = ok & (wt > 0.0)
                joined |= ok
            total = np.where(ok[..., None], total + wt[..., None] * e_q, total)
            wsum = np.where(ok, wsum + wt, wsum)
    out = total / wsum[..., None]
    return np.where((centre_ok & joined)[..., None], out, e).astype(F)


def denoise(mean, guides, params, tonemap_op, oracle):
    """rpt_denoise / rpt_debug_denoise_host: mean (H, W, 3) f32, guides as Renderer.guides() returns them, params with the fields of rpt_denoise_params"""
    expr = lambda x: oracle.math(3, np.ascontiguousarray(x, F))
    mean = np.ascontiguousarray(mean, F)
    albedo = np.ascontiguousarray(guides["albedo"], F)
    normal, position = np.ascontiguousarray(guides["normal"], F), np.ascontiguousarray(guides["position"], F)
    depth, kind = np.ascontiguousarray(guides["depth"], F), np.ascontiguousarray(guides["kind"], np.uint32)
    demodulated = params.iterations != 0 and params.demodulate != 0
    with np.errstate(all="ignore"):
        e = (mean / albedo_floor(albedo)).astype(F) if demodulated else mean
        for i in range(params.iterations):
            e = filter_pass(e, normal, position, depth, kind, i, params.normal_power_log2, params.sigma_color, params.sigma_plane, expr)
        if demodulated:
            e = (e * albedo_floor(albedo)).astype(F)
    return tonemap(e, tonemap_op, oracle)


def tonemap(rgb, op, oracle):
    """the display operator on an (H, W, 3) image: oracle.resolve with a sample count of 1 (x / 1 = x)"""
    acc = np.zeros(rgb.shape[:2] + (4,), F)
    acc[..., :3] = rgb
    acc[..., 3] = 1.0
    return oracle.resolve(acc, 1.0, op)


# ---- guides ---------------------------------------------------------------------------------------------------------------------------------------

def camera_rays(cfg, oracle):
    """camera_ray (lib.rs:36-51) with the jitter replaced by (0.5, 0.5): origins, directions as (H * W, 3), row-major pixels"""
    w, h = cfg.width, cfg.height
    ys, xs = np.mgrid[0:h, 0:w]
    sx, sy = xs.astype(F) + F(0.5), ys.astype(F) + F(0.5)
    ux = (sx / F(w)) * F(2.0) - F(1.0)
    uy = (F(1.0) - sy / F(h)) * F(2.0) - F(1.0)
    uy = uy * (F(h) / F(w))
    v = np.stack([ux, uy, np.ones_like(ux)], -1).astype(F)
    v = v * (F(1.0) / np.sqrt(dot3(v, v)))[..., None]
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


def sample_atlas(atlas_u8, u, v):
    """the CPU polyfill's bilinear sampler (image_polyfill.rs:32-55) on the RGBA8 atlas: texel = u8 / 255"""
    ah, aw = atlas_u8.shape[:2]
    sx, sy = (u * F(aw)).astype(F), (v * F(ah)).astype(F)
    fx, fy = np.floor(sx), np.floor(sy)
    tx, ty = (sx - fx)[..., None], (sy - fy)[..., None]
    x0, y0 = fx.astype(np.int64) % aw, fy.astype(np.int64) % ah
    x1, y1 = np.ceil(sx).astype(np.int64) % aw, np.ceil(sy).astype(np.int64) % ah
    tex = lambda y, x: (atlas_u8[y, x, :3].astype(F) / F(255.0)).astype(F)
    c00, c10, c01, c11 = tex(y0, x0), tex(y0, x1), tex(y1, x0), tex(y1, x1)
    a = c00 + (c10 - c00) * tx
    b = c01 + (c11 - c01) * tx
    return (a + (b - a) * ty).astype(F)


def guides(world, cfg, oracle, oracle_scene=None):
    """the guide buffers of csrc/k_denoise.h from the oracle's nearest hits and the scene arrays, in the layout of Renderer.guides()"""
    w, h = cfg.width, cfg.height
    scene = oracle_scene if oracle_scene is not None else oracle.scene(world)
    ro, rd = camera_rays(cfg, oracle)
    t, tri, flags, _ = oracle.trace_rays(scene, 0, ro, rd)
    hit = (flags & 1) != 0
    with np.errstate(all="ignore"):
        position = (ro + rd * t[:, None]).astype(F)
        kind = np.zeros(len(t), np.uint32)
        albedo = np.ones((len(t), 3), F)
        normal = np.zeros((len(t), 3), F)
        idx = world.indices[np.where(hit, tri, 0)]
        mat = world.materials[idx["material"]]
        emits = (mat["emissive"][:, :3] != 0).any(axis=1)
        kind[hit] = np.where(emits[hit], KIND_EMITTER, KIND_SURFACE)
        pa, pb, pc = (world.per_vertex[idx[k]] for k in ("v0", "v1", "v2"))
        a3 = pa["vertex"][:, :3]
        v0, v1, v2 = pb["vertex"][:, :3] - a3, pc["vertex"][:, :3] - a3, position - a3
        d00, d01, d11, d20, d21 = dot3(v0, v0), dot3(v0, v1), dot3(v1, v1), dot3(v2, v0), dot3(v2, v1)
        denom = d00 * d11 - d01 * d01
        bv = (d11 * d20 - d01 * d21) / denom
        bw = (d00 * d21 - d01 * d20) / denom
        bu = F(1.0) - bv - bw
        interp = lambda f, n: bu[:, None] * pa[f][:, :n] + bv[:, None] * pb[f][:, :n] + bw[:, None] * pc[f][:, :n]
        nrm = interp("normal", 3).astype(F)
        surf_albedo = mat["albedo"][:, :3].astype(F)
        atlas = getattr(world, "atlas", None)
        if atlas is not None:
            uv = ((bu[:, None] * pa["uv0"] + bv[:, None] * pb["uv0"]) + bw[:, None] * pc["uv0"]).astype(F)
            wrap = (np.clip(uv, 0, 1) != uv).any(axis=1)
            uv = np.where(wrap[:, None], uv - np.floor(uv), uv).astype(F)
            has_n = mat["has_normal_texture"] != 0
            nm = sample_atlas(atlas, mat["normals"][:, 0] + uv[:, 0] * mat["normals"][:, 2], mat["normals"][:, 1] + uv[:, 1] * mat["normals"][:, 3]) * F(2.0) - F(1.0)
            tangent = interp("tangent", 3).astype(F)
            bitangent = np.cross(tangent, nrm).astype(F)
            mapped = tangent * nm[:, 0:1] + bitangent * nm[:, 1:2] + nrm * nm[:, 2:3]
            mapped = (mapped * (F(1.0) / np.sqrt(dot3(mapped, mapped)))[:, None]).astype(F)      # lib.rs:141; the guide normalises once more below
            nrm = np.where(has_n[:, None], mapped, nrm).astype(F)
            has_a = mat["has_albedo_texture"] != 0
            tex_a = sample_atlas(atlas, mat["albedo"][:, 0] + uv[:, 0] * mat["albedo"][:, 2], mat["albedo"][:, 1] + uv[:, 1] * mat["albedo"][:, 3])
            surf_albedo = np.where(has_a[:, None], tex_a, surf_albedo).astype(F)
        nrm = (nrm * (F(1.0) / np.sqrt(dot3(nrm, nrm)))[:, None]).astype(F)
        nrm = np.where(finite3(nrm)[:, None], nrm, F(0.0)).astype(F)
        normal[hit] = nrm[hit]
        surface = hit & ~emits
        albedo[surface] = surf_albedo[surface]
    return {"albedo": albedo.reshape(h, w, 3), "normal": normal.reshape(h, w, 3), "position": position.reshape(h, w, 3),
            "depth": t.reshape(h, w).copy(), "kind": kind.reshape(h, w)}


# ---- quality ---------------------------------------------------------------------------------------------------------------------------------------

QUALITY = [("DarkCornell", 0), ("VeachMIS", 1), ("PBRTest", 0)]


def quality_images(rpt, world, oracle, scene, nee, noisy_spp=8, converged_spp=1024):
    W = H = 128
    cfg = rpt.default_config(W, H, nee=nee)
    w = world(scene)
    sc = oracle.scene(w)
    seeds = rpt.blue_noise_seeds(W, H)
    noisy, rng, _ = oracle.trace_cpu(cfg, sc, seeds, noisy_spp)
    conv, _, _ = oracle.trace_cpu(cfg, sc, rng, converged_spp - noisy_spp, accum=noisy)      # the 1024-spp image continues the 8-spp one
    return ((noisy[..., :3] / np.float32(noisy_spp)).astype(np.float32), (conv[..., :3] / np.float32(converged_spp)).astype(np.float32),
            guides(w, cfg, oracle, sc))
