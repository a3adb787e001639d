"""numpy restatement, in f32 and in the same operation order, of the temporal stage of csrc/k_temporal.h (tp_project, tp_tap, tp_reproject, tp_pixel) in front
of the variance-guided passes of tests/denoise_var_ref.py.

Not a test module (no test_ prefix): tests/test_denoise_temporal.py holds the host build against it.  As in tests/denoise_ref.py the sine and cosine of the
camera rotation are the oracle's (oracle.math(0 / 1, .)); everything else here is plain IEEE f32 arithmetic, which numpy performs operation by operation
without fusing.  `project64` is the same projection in float64 from the cameras' angles, for the one accuracy check.
"""
import numpy as np

import denoise_ref
import denoise_var_ref
from denoise_ref import F, KIND_MISS, albedo_floor, dot3, finite3

INF = F(np.inf)


def camera_matrix(cfg, oracle):
    """DevConfig::euler: the columns of RotY(yaw) * RotX(pitch), as (3, 3) with m[c] = column c (the loop of denoise_ref.camera_rays)"""
    sin = lambda a: oracle.math(0, np.array([a], F))[0]
    cos = lambda a: oracle.math(1, np.array([a], F))[0]
    sy_, cy_ = sin(cfg.cam_rotation[1]), cos(cfg.cam_rotation[1])
    sx_, cx_ = sin(cfg.cam_rotation[0]), cos(cfg.cam_rotation[0])
    z, o = F(0.0), F(1.0)
    ry = np.array([[cy_, z, -sy_], [z, o, z], [sy_, z, cy_]], F)
    rx = np.array([[o, z, z], [z, cx_, sx_], [z, -sx_, cx_]], F)
    m = np.zeros((3, 3), F)
    for c in range(3):
        for r in range(3):
            acc = F(ry[0][r] * rx[c][0])
            acc = F(acc + F(ry[1][r] * rx[c][1]))
            acc = F(acc + F(ry[2][r] * rx[c][2]))
            m[c][r] = acc
    return m


def camera_position(cfg):
    return np.array(list(cfg.cam_position)[:3], F)


def project(position, kind, ro_cur, ro_prev, euler_prev, w, h):
    """tp_project for every pixel: (fx, fy, ok)"""
    o = np.where((kind == KIND_MISS)[..., None], ro_cur, ro_prev).astype(F)
    r = (position - o).astype(F)
    d = [dot3(np.broadcast_to(euler_prev[c], r.shape), r).astype(F) for c in range(3)]
    ok = d[2] > F(0.0)
    ux = d[0] / d[2]
    uy = (d[1] / d[2]) / F(F(h) / F(w))
    sx = ((ux + F(1.0)) / F(2.0)) * F(w)
    sy = (F(1.0) - (uy + F(1.0)) / F(2.0)) * F(h)
    fx, fy = (sx - F(0.5)).astype(F), (sy - F(0.5)).astype(F)
    ok = ok & (fx > F(-1.0)) & (fx < F(w)) & (fy > F(-1.0)) & (fy < F(h))
    return fx, fy, ok


def project64(position, kind, cfg_cur, cfg_prev):
    """the projection in float64, rotation from the angles in float64: (fx, fy, in front of the previous camera)"""
    w, h = cfg_cur.width, cfg_cur.height
    yaw, pitch = float(cfg_prev.cam_rotation[1]), float(cfg_prev.cam_rotation[0])
    ry = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])             # rows: the matrix itself
    rx = np.array([[1, 0, 0], [0, np.cos(pitch), -np.sin(pitch)], [0, np.sin(pitch), np.cos(pitch)]])
    m = ry @ rx
    o = np.where((kind == KIND_MISS)[..., None], np.array(list(cfg_cur.cam_position)[:3], np.float64), np.array(list(cfg_prev.cam_position)[:3], np.float64))
    d = (position.astype(np.float64) - o) @ m                                                              # m^T r
    with np.errstate(all="ignore"):
        ux, uy = d[..., 0] / d[..., 2], (d[..., 1] / d[..., 2]) / (h / w)
        return (ux + 1) / 2 * w - 0.5, (1 - (uy + 1) / 2) * h - 0.5, d[..., 2] > 0


def reproject(guides, previous, view, params):
    """tp_reproject for every pixel: (reusable, e_r, n_r, mu1_r, mu2_r).  previous: {"normal", "position", "kind", "records"}; view: (ro_cur, ro_prev,
    euler_prev, identity)"""
    normal, position, depth, kind = guides["normal"], guides["position"], guides["depth"], guides["kind"]
    h, w = kind.shape
    ro_cur, ro_prev, euler_prev, identity = view
    rec = previous["records"]
    plane = (F(F(2.0) / F(w)) * depth).astype(F)
    ys, xs = np.mgrid[0:h, 0:w]
    se = np.zeros((h, w, 3), F)
    sn, s1, s2, wt = (np.zeros((h, w), F) for _ in range(4))
    if identity:
        live = np.ones((h, w), bool)
        taps = [(xs, ys, np.ones((h, w), F))]
    else:
        fx, fy, live = project(position, kind, ro_cur, ro_prev, euler_prev, w, h)
        fx, fy = np.where(live, fx, F(0.0)).astype(F), np.where(live, fy, F(0.0)).astype(F)
        x0f, y0f = np.floor(fx), np.floor(fy)
        a, b = (fx - x0f).astype(F), (fy - y0f).astype(F)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        ia, ib = (F(1.0) - a).astype(F), (F(1.0) - b).astype(F)
        taps = [(x0, y0, ia * ib), (x0 + 1, y0, a * ib), (x0, y0 + 1, ia * b), (x0 + 1, y0 + 1, a * b)]
    hit = kind != KIND_MISS
    for qx, qy, wq in taps:
        inside = (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
        qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
        r = rec[qy, qx]
        ok = live & inside & (r[..., 3] > F(0.0)) & (previous["kind"][qy, qx] == kind)
        ndot = dot3(normal, previous["normal"][qy, qx])
        dist = np.abs(dot3(normal, (previous["position"][qy, qx] - position).astype(F))) / plane
        ok = ok & (~hit | ((ndot >= F(params.normal_min)) & (dist <= F(params.plane_max))))
        wq = wq.astype(F)
        se = np.where(ok[..., None], se + wq[..., None] * r[..., :3], se).astype(F)
        sn = np.where(ok, sn + wq * r[..., 3], sn).astype(F)
        s1 = np.where(ok, s1 + wq * r[..., 4], s1).astype(F)
        s2 = np.where(ok, s2 + wq * r[..., 5], s2).astype(F)
        wt = np.where(ok, wt + wq, wt).astype(F)
    usable = wt > F(0.01)
    den = np.where(usable, wt, F(1.0))
    e_r, mu1_r, mu2_r = (se / den[..., None]).astype(F), (s1 / den).astype(F), (s2 / den).astype(F)
    n = (sn / den).astype(F)
    n_r = np.where(n > F(params.max_history), F(params.max_history), n).astype(F)
    return usable & (n_r > F(0.0)), e_r, n_r, mu1_r, mu2_r


def blend(mean, guides, moments, previous, view, params, demodulated):
    """tp_pixel for every pixel: (e, v, T, records (H, W, 6), reused)"""
    albedo = guides["albedo"]
    h, w = guides["kind"].shape
    e_cur = (mean / albedo_floor(albedo)).astype(F) if demodulated else mean
    n_cur = moments[..., 2]
    v0 = denoise_var_ref.prepare_variance(moments, demodulated, albedo)
    mu1_0, mu2_0 = (moments[..., 0] / n_cur).astype(F), (moments[..., 1] / n_cur).astype(F)
    reused = np.zeros((h, w), bool)
    if previous is not None:
        reused, e_r, n_r, mu1_r, mu2_r = reproject(guides, previous, view, params)
        reused = reused & finite3(e_cur)
    if not reused.any():
        e, v, T, mu1, mu2 = e_cur, v0, n_cur, mu1_0, mu2_0
    else:
        T1 = (n_r + n_cur).astype(F)
        e1 = ((n_r[..., None] * e_r + n_cur[..., None] * e_cur) / T1[..., None]).astype(F)
        sums = np.isfinite(moments[..., 0]) & np.isfinite(moments[..., 1])
        mu1_1 = ((n_r * mu1_r + np.where(sums, moments[..., 0], F(0.0))) / T1).astype(F)
        mu2_1 = ((n_r * mu2_r + np.where(sums, moments[..., 1], F(0.0))) / T1).astype(F)
        known = (T1 >= F(2.0)) & np.isfinite(mu1_1) & np.isfinite(mu2_1)
        ss = (mu2_1 - mu1_1 * mu1_1).astype(F)
        v1 = (np.where(ss > F(0.0), ss, F(0.0)).astype(F) / (T1 - F(1.0))).astype(F)
        if demodulated:
            ya = denoise_var_ref.luminance(albedo_floor(albedo)).astype(F)
            v1 = np.where(np.isfinite(v1), v1 / (ya * ya), v1).astype(F)
        v1 = np.where(known, v1, INF).astype(F)
        e = np.where(reused[..., None], e1, e_cur).astype(F)
        v, T = np.where(reused, v1, v0).astype(F), np.where(reused, T1, n_cur).astype(F)
        mu1, mu2 = np.where(reused, mu1_1, mu1_0).astype(F), np.where(reused, mu2_1, mu2_0).astype(F)
    records = np.concatenate([e, np.where(finite3(e), T, F(0.0)).astype(F)[..., None], mu1[..., None], mu2[..., None]], -1).astype(F)
    return e, v, T, records, reused


def denoise_temporal(mean, guides, moments, camera, previous, params, tonemap_op, oracle):
    """rpt_denoise_temporal / rpt_debug_denoise_temporal_host: the arguments of hip.denoise_temporal_host; returns the same dictionary"""
    expr = lambda x: oracle.math(3, np.ascontiguousarray(x, F))
    g = {k: np.ascontiguousarray(guides[k], np.uint32 if k == "kind" else F) for k in ("albedo", "normal", "position", "depth", "kind")}
    mean, moments = np.ascontiguousarray(mean, F), np.ascontiguousarray(moments, F)
    b = params.filter.base
    demodulated = b.iterations != 0 and b.demodulate != 0
    view = None
    if previous is not None:
        previous = {k: np.ascontiguousarray(previous[k], np.uint32 if k == "kind" else F) for k in ("normal", "position", "kind", "records")} | {"camera": previous["camera"]}
        ro_cur, ro_prev = camera_position(camera), camera_position(previous["camera"])
        m_cur, m_prev = camera_matrix(camera, oracle), camera_matrix(previous["camera"], oracle)
        identity = ro_cur.tobytes() == ro_prev.tobytes() and m_cur.tobytes() == m_prev.tobytes()
        view = (ro_cur, ro_prev, m_prev, identity)
    with np.errstate(all="ignore"):
        e, v, T, records, reused = blend(mean, g, moments, previous, view, params, demodulated)
        for i in range(b.iterations):
            e, v = denoise_var_ref.filter_pass_var(e, v, g["normal"], g["position"], g["depth"], g["kind"], i, b.normal_power_log2, b.sigma_color, b.sigma_plane,
                                                   params.filter.sigma_variance, expr)
        if demodulated:
            e = (e * albedo_floor(g["albedo"])).astype(F)
    return {"rgb": denoise_ref.tonemap(e, tonemap_op, oracle), "variance": v, "history": T, "records": records, "pixels_with_history": int(reused.sum())}
