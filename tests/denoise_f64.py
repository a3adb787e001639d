"""An independent float64 statement of the denoisers and of the noise estimate: rpt_denoise, rpt_denoise_variance, rpt_denoise_temporal, the variance of
the mean and noise_rel.  Written from the formulas of DESIGN.md (N5, N6, N8, N9) and of the header comments of csrc/k_denoise.h, csrc/k_temporal.h and
csrc/k_moments.h — not from their loops, and not from tests/denoise_ref.py, denoise_var_ref.py, temporal_ref.py or moments_ref.py, none of which is
imported here.  Whole-image shifts instead of per-pixel tap loops; sums in whatever order numpy takes; numpy.exp, numpy.cos and numpy.sin on the angles.

Not a test module.  It takes what the host hooks take (f32 arrays, widened on entry; the parameter structs; the cameras) and keeps every intermediate in
float64 across all passes.  The constants the design states as f32 literals (the luminance weights, the floors 0.01, 1e-6 and 1e-12) are those f32 values.
The display operators are f64_ref.resolve's.

Rules for what is not finite, as documented: a centre that is not finite passes through; a tap that is not finite is skipped; an unknown variance is
+inf; a pixel no tap joined passes through.  "Finite" is what f32 calls finite, so a float64 intermediate beyond the f32 range counts as infinite.

Where f32 and float64 can legitimately decide differently the functions return what a caller needs to leave such pixels out: `temporal` a margin per
pixel (the smallest distance of a decision from its threshold), the filters a flag for pixels whose luminance term is ill-conditioned.  Error bounds are
not worked out here: a caller may pass an observer (`watch`) that is shown the quantities of every pass and changes nothing.
"""
import numpy as np

import f64_ref
from f64_ref import f32

INF = np.inf
WR, WG, WB = f32(0.2126), f32(0.7152), f32(0.0722)
ALBEDO_FLOOR = f32(0.01)
MEAN_FLOOR = f32(0.01)
WIDTH_FLOOR = f32(1e-6)
COLOUR_FLOOR = f32(1e-12)
F32_MAX = float(np.finfo(np.float32).max)
U = 2.0 ** -24                                   # the unit roundoff of f32
H5 = {-2: 1.0 / 16, -1: 1.0 / 4, 0: 3.0 / 8, 1: 1.0 / 4, 2: 1.0 / 16}
H3 = {-1: 1.0 / 4, 0: 1.0 / 2, 1: 1.0 / 4}
KIND_MISS = 0
# a bilinear tap lighter than this decides nothing worth a margin: toggling it moves Wt and every weighted mean by at most this share
TAP_MIN = 1e-6
# the luminance flag (see filter_variance): a tap is at risk where the width is below LUM_K roundoffs of the two luminances, and it counts where it
# could carry more than LUM_SHARE of the centre's weight sum
LUM_K = 4096.0
LUM_SHARE = 1e-4


def widen(a):
    return np.asarray(a, np.float64)


def finite(a):
    """finite as f32 sees it"""
    with np.errstate(invalid="ignore"):
        return np.abs(a) <= F32_MAX


def finite3(a):
    return finite(a).all(axis=-1)


def luminance(c):
    with np.errstate(invalid="ignore"):                              # (inf - inf among hostile inputs: a NaN, which every user of it masks)
        return WR * c[..., 0] + WG * c[..., 1] + WB * c[..., 2]


def dot(a, b):
    return (a * b).sum(axis=-1)


# ---- N6: the moments record ---------------------------------------------------------------------------------------------------------------------------

def measured(moments):
    m = widen(moments)
    with np.errstate(invalid="ignore"):
        return (m[..., 2] >= 2.0) & finite(m[..., 0]) & finite(m[..., 1])


def variance_of_mean(moments):
    """max(0, sum(Y^2) - sum(Y)^2 / n) / (n (n - 1)); +inf (unknown) below two samples or where a sum is not finite"""
    m = widen(moments)
    n = m[..., 2]
    with np.errstate(all="ignore"):
        v = np.maximum(m[..., 1] - m[..., 0] ** 2 / n, 0.0) / (n * (n - 1.0))
    return np.where(measured(m), v, INF)


def noise_rel(moments):
    """the standard error of the mean luminance over (|mean| + 0.01); +inf where the variance is unknown"""
    m = widen(moments)
    with np.errstate(all="ignore"):
        rel = np.sqrt(variance_of_mean(m)) / (np.abs(m[..., 0] / m[..., 2]) + MEAN_FLOOR)
    return np.where(measured(m), rel, INF)


def moments_of_samples(radiance):
    """(sum Y, sum Y^2, n) in float64 of per-sample radiances (n, ..., 3)"""
    y = luminance(widen(radiance))
    return np.stack([y.sum(axis=0), (y * y).sum(axis=0), np.full(y.shape[1:], float(len(y)))], -1)


# ---- N5 / N8: the filters ------------------------------------------------------------------------------------------------------------------------------

def shifted(a, dy, dx, fill=0.0):
    """b[y, x] = a[y + dy, x + dx] where that is inside the image, `fill` elsewhere"""
    h, w = a.shape[:2]
    out = np.full(a.shape, fill, a.dtype)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def inside(h, w, dy, dx):
    return shifted(np.ones((h, w), bool), dy, dx, False)


def guide_arrays(guides):
    return {k: (np.asarray(guides[k]).astype(np.int64) if k == "kind" else widen(guides[k])) for k in ("albedo", "normal", "position", "depth", "kind")}


def albedo_floor(albedo):
    return np.maximum(albedo, ALBEDO_FLOOR)


def prefiltered_variance(v, kind, plane=None):
    """vbar: the 3 x 3 Gaussian {1/4, 1/2, 1/4}^2 of v at distance 1 over the taps inside the image, of the centre's kind and of known variance, over the
    weights used; +inf where there is none.  plane: averaged in v's place, over v's taps."""
    h, w = v.shape
    acc, ksum = np.zeros((h, w)), np.zeros((h, w))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            v_q = shifted(v, dy, dx, INF)
            ok = inside(h, w, dy, dx) & (shifted(kind, dy, dx, -1) == kind) & finite(v_q)
            k = H3[dy] * H3[dx]
            acc += np.where(ok, k * (np.where(ok, v_q, 0.0) if plane is None else shifted(plane, dy, dx)), 0.0)
            ksum += np.where(ok, k, 0.0)
    with np.errstate(all="ignore"):
        return np.where(ksum > 0.0, acc / ksum, INF)


def one_pass(e, v, g, i, base, sigma_variance, tainted, watch=None):
    """pass i (step 2^i) of the a-trous filter over the colour e (H, W, 3) and, where v is not None, the variance v (H, W).  Returns e, v and the
    pixels that are tainted afterwards: flagged in this pass (filter_variance says how), or fed by a tainted tap with more than LUM_SHARE of their weight
    sum.  watch: an observer that is shown the pass's quantities (start, every tap, finish) and changes nothing; tests/denoise_f64_cases.py carries an error
    bound of the variance through the passes that way."""
    h, w = e.shape[:2]
    step = 1 << i
    normal, position, depth, kind = g["normal"], g["position"], g["depth"], g["kind"]
    hit = kind != KIND_MISS
    centre_ok = finite3(e)
    sigma_i = float(base.sigma_color) * 2.0 ** -i
    plane = (float(base.sigma_plane) * step * (2.0 / w)) * depth
    lum = luminance(e)
    term = vbar = width = None
    if v is not None and float(sigma_variance) != 0.0:
        vbar = prefiltered_variance(v, kind)
        term = finite(vbar)
        with np.errstate(all="ignore"):
            width = float(sigma_variance) * np.sqrt(np.where(term, vbar, 0.0)) + WIDTH_FLOOR       # inf * 0 = NaN where vbar = 0: every weight NaN, nothing joins
    if watch is not None:
        watch.start(i=i, e=e, v=v, kind=kind, centre_ok=centre_ok, sigma_i=sigma_i, sigma_variance=float(sigma_variance), term=term, vbar=vbar, width=width)
    k0 = H5[0] * H5[0]                             # the centre always counts with its kernel weight
    sum_e, wsum = k0 * np.where(centre_ok[..., None], e, 0.0), np.full((h, w), k0)
    vsum = np.zeros((h, w)) if v is None else np.where(finite(v), k0 * k0 * np.where(finite(v), v, 0.0), 0.0)
    joined = np.zeros((h, w), bool)
    risk_weight = np.zeros((h, w))                 # the largest weight an at-risk tap can have on either side
    taint_weight = np.zeros((h, w))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if dy == 0 and dx == 0:
                continue
            oy, ox = dy * step, dx * step
            if abs(oy) >= h or abs(ox) >= w:
                continue
            e_q = shifted(e, oy, ox, np.nan)
            ok = inside(h, w, oy, ox) & (shifted(kind, oy, ox, -1) == kind) & finite3(e_q) & centre_ok
            e_q = np.where(ok[..., None], e_q, 0.0)
            e_p = np.where(ok[..., None], e, 0.0)
            d_c = d_l = np.zeros((h, w))
            y_p = y_q = None
            with np.errstate(all="ignore"):
                w_n = np.maximum(0.0, dot(normal, shifted(normal, oy, ox))) ** (2 ** int(base.normal_power_log2))
                d_x = np.abs(dot(normal, shifted(position, oy, ox) - position)) / plane
                w_n, d_x = np.where(hit, w_n, 1.0), np.where(hit, d_x, 0.0)
                if sigma_i != 0.0:
                    diff = e_p - e_q
                    d_c = dot(diff, diff) / (sigma_i ** 2 * (dot(e_p, e_p) + dot(e_q, e_q) + COLOUR_FLOOR))
                k = H5[dy] * H5[dx]
                if term is not None:
                    y_q = np.where(ok, shifted(lum, oy, ox), 0.0)
                    y_p = np.where(ok, lum, 0.0)
                    d_l = np.where(term, np.abs(y_p - y_q) / width, 0.0)
                    doubt = LUM_K * U * (np.abs(y_p) + np.abs(y_q))                                 # what |Y_p - Y_q| may be off by on the f32 side
                    at_risk = ok & term & (width < doubt)                                           # (a NaN width: nothing joins on either side)
                    w_most = k * w_n * np.exp(-(d_x + d_c + np.maximum(0.0, np.abs(y_p - y_q) - doubt) / width))
                    risk_weight = np.maximum(risk_weight, np.where(at_risk & (w_most > 0.0), w_most, 0.0))
                wq = k * w_n * np.exp(-(d_x + d_c + d_l))
                live = ok & (wq > 0.0)                                                             # a NaN is not > 0
            wq = np.where(live, wq, 0.0)
            joined |= live
            sum_e += wq[..., None] * e_q
            wsum += wq
            v_q = known_q = None
            if v is not None:
                v_q = shifted(v, oy, ox, INF)
                known_q = live & finite(v_q)
                vsum += np.where(known_q, wq * wq * np.where(known_q, v_q, 0.0), 0.0)
            if tainted is not None:
                taint_weight += np.where(shifted(tainted, oy, ox, False), wq, 0.0)
            if watch is not None:
                watch.tap(oy=oy, ox=ox, ok=ok, live=live, wq=wq, e_p=e_p, e_q=e_q, d_x=d_x, d_c=d_c, d_l=d_l, y_p=y_p, y_q=y_q, v_q=v_q, known_q=known_q)
    with np.errstate(all="ignore"):
        out_e = np.where(joined[..., None], sum_e / wsum[..., None], e)
        out_v = None if v is None else np.where(joined, np.where(finite(v), vsum / wsum ** 2, INF), v)
    if watch is not None:
        watch.finish(joined=joined, wsum=wsum, e=e, v=v, out_e=out_e, out_v=out_v)
    flagged = risk_weight > LUM_SHARE * wsum
    if tainted is not None:
        flagged = flagged | tainted | (taint_weight > LUM_SHARE * wsum)
    return out_e, out_v, flagged


def _finish(e, albedo, demodulated, op):
    with np.errstate(all="ignore"):
        return f64_ref.resolve(e * albedo_floor(albedo) if demodulated else e, 1.0, op)


def _passes(e, v, g, base, sigma_variance, watch=None):
    flagged = np.zeros(e.shape[:2], bool)
    for i in range(int(base.iterations)):
        e, v, flagged = one_pass(e, v, g, i, base, sigma_variance, flagged, watch)
    return e, v, flagged


def filter(mean, guides, params, op=0):
    """rpt_denoise: -> rgb (H, W, 3)"""
    g = guide_arrays(guides)
    demodulated = params.iterations != 0 and params.demodulate != 0
    with np.errstate(all="ignore"):
        e = widen(mean) / albedo_floor(g["albedo"]) if demodulated else widen(mean)
    e, _, _ = _passes(e, None, g, params, 0.0)
    return _finish(e, g["albedo"], demodulated, op)


def prepared_variance(v, albedo, demodulated):
    """the variance in the filter's units: over Ya^2, Ya the luminance of max(albedo, 0.01), where the image is demodulated; unknown stays unknown"""
    if not demodulated:
        return v
    with np.errstate(all="ignore"):
        return np.where(finite(v), v / luminance(albedo_floor(albedo)) ** 2, INF)


def filter_variance(mean, guides, moments, params, op=0, watch=None):
    """rpt_denoise_variance: -> rgb (H, W, 3), variance (H, W), flagged (H, W): pixels whose luminance term is ill-conditioned, or that such pixels feed.
    watch: an observer (see one_pass); it is shown the prepared colour and variance first.

    The flag.  d_l = |Y_p - Y_q| / width divides a difference of two f32 luminances by a width that can be as small as 1e-6.  On the f32 side the
    difference is off by some roundoffs of |Y_p| + |Y_q| — the luminance's own three products and two sums, and from the second pass on the rounding of
    the earlier passes' sums (a few tens of roundoffs for 25 taps and a quotient per pass) — so a tap is at risk where width < LUM_K 2^-24 (|Y_p| +
    |Y_q|): d_l is then in doubt by more than one unit.  It counts while the tap can still carry more than LUM_SHARE of the centre's weight sum: by its
    float64 weight with |Y_p - Y_q| reduced by that doubt, which is its float64 weight wherever the two luminances agree to within the doubt, and
    nothing where they differ by more (a dead tap on either side).  Dead taps (another kind, not finite, outside, a zero normal weight) do not
    count.  A flagged pixel taints, in the later passes, every centre that takes more than LUM_SHARE of its weight sum from it.  All of it from float64
    values alone."""
    g = guide_arrays(guides)
    b = params.base
    demodulated = b.iterations != 0 and b.demodulate != 0
    with np.errstate(all="ignore"):
        e = widen(mean) / albedo_floor(g["albedo"]) if demodulated else widen(mean)
    v = prepared_variance(variance_of_mean(moments), g["albedo"], demodulated)
    if watch is not None:
        watch.prepared(e=e, v=v, scale=lambda plane: prepared_variance(plane, g["albedo"], demodulated))
    e, v, flagged = _passes(e, v, g, b, params.sigma_variance, watch)
    return _finish(e, g["albedo"], demodulated, op), v, flagged


def passes(e, v, guides, params, op=0, watch=None):
    """the passes and the finish of rpt_denoise_variance alone, from a colour e and a variance v that are in the filter's units already (what temporal reuse
    hands to them): -> rgb, variance, flagged"""
    g = guide_arrays(guides)
    b = params.base
    demodulated = b.iterations != 0 and b.demodulate != 0
    e, v, flagged = _passes(widen(e), widen(v), g, b, params.sigma_variance, watch)
    return _finish(e, g["albedo"], demodulated, op), v, flagged


# ---- N9: temporal reuse --------------------------------------------------------------------------------------------------------------------------------

def camera_rotation(cfg):
    """RotY(yaw) RotX(pitch): camera space to world space"""
    return f64_ref.rotation_y(float(cfg.cam_rotation[1])) @ f64_ref.rotation_x(float(cfg.cam_rotation[0]))


def camera_position(cfg):
    return np.array([float(cfg.cam_position[k]) for k in range(3)])


def same_camera(a, b):
    """position and rotation equal word for word: the identity path"""
    words = lambda c: np.array([c.cam_position[k] for k in range(3)] + [c.cam_rotation[k] for k in range(2)], np.float32).tobytes()
    return words(a) == words(b)


def reproject(position, kind, camera, previous_camera, width, height):
    """the screen position, minus half a pixel, of every world position in the previous view: hits from the previous camera's origin, misses (the sky is
    at infinity) from the current one.  -> fx, fy, usable (in front and inside (-1, W) x (-1, H)), front (d.z relative to |x - o|)"""
    x = widen(position)
    o = np.where((np.asarray(kind) == KIND_MISS)[..., None], camera_position(camera), camera_position(previous_camera))
    r = x - o
    d = r @ camera_rotation(previous_camera)                        # R^T r: world to the previous camera's space
    with np.errstate(all="ignore"):
        ux = d[..., 0] / d[..., 2]
        uy = (d[..., 1] / d[..., 2]) / (height / width)
        fx = (ux + 1.0) / 2.0 * width - 0.5
        fy = (1.0 - (uy + 1.0) / 2.0) * height - 0.5
        front = d[..., 2] / np.sqrt(dot(r, r))
        usable = (d[..., 2] > 0.0) & (fx > -1.0) & (fx < width) & (fy > -1.0) & (fy < height)
    return fx, fy, usable, front


def temporal(mean, guides, moments, camera, previous, params, op=0, watch=None):
    """rpt_denoise_temporal.  previous: None or {"camera", "normal", "position", "kind", "records" (H, W, 6): e_h.rgb, N, mu1, mu2}.
    -> {"rgb", "variance", "history" (T), "records", "reused", "pixels_with_history", "margin", "flagged"}.

    margin (H, W): the smallest, over the decisions a pixel takes, of the distance from the threshold — |n_p . n_q - normal_min| and |dist - plane_max| /
    max(1, plane_max) for the taps whose bilinear weight exceeds TAP_MIN and that the exact rules (inside, N > 0, kind) let through, |Wt - 0.01|, |T - 2|,
    and d.z / |x_p - o|.  On the identity path the one tap has weight 1 and Wt and T involve no rounding, so only the tap's two tests count.

    watch: an observer (see one_pass); it is shown the blend first — the four taps of every pixel and what came of them."""
    g = guide_arrays(guides)
    h, w = g["kind"].shape
    b = params.filter.base
    demodulated = b.iterations != 0 and b.demodulate != 0
    m = widen(moments)
    n_cur = m[..., 2]
    with np.errstate(all="ignore"):
        e_cur = widen(mean) / albedo_floor(g["albedo"]) if demodulated else widen(mean)
        mu1, mu2 = m[..., 0] / n_cur, m[..., 1] / n_cur
    v = prepared_variance(variance_of_mean(m), g["albedo"], demodulated)
    e, T = e_cur, n_cur
    reused = np.zeros((h, w), bool)
    margin = np.full((h, w), INF)
    seen = None
    if previous is not None:
        rec = widen(previous["records"])
        pn, pp, pk = widen(previous["normal"]), widen(previous["position"]), np.asarray(previous["kind"]).astype(np.int64)
        normal_min, plane_max, max_history = float(params.normal_min), float(params.plane_max), float(params.max_history)
        hit = g["kind"] != KIND_MISS
        ys, xs = np.mgrid[0:h, 0:w]
        identity = same_camera(camera, previous["camera"])
        if identity:
            live = np.ones((h, w), bool)
            taps = [(xs, ys, np.ones((h, w)))]
        else:
            fx, fy, live, front = reproject(g["position"], g["kind"], camera, previous["camera"], w, h)
            margin = np.minimum(margin, np.where(np.isnan(front), 0.0, np.abs(front)))
            fx, fy = np.where(live, fx, 0.0), np.where(live, fy, 0.0)
            x0, y0 = np.floor(fx), np.floor(fy)
            a, bb = fx - x0, fy - y0
            x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
            taps = [(x0, y0, (1 - a) * (1 - bb)), (x0 + 1, y0, a * (1 - bb)), (x0, y0 + 1, (1 - a) * bb), (x0 + 1, y0 + 1, a * bb)]
        joined_taps = []
        s_e, s_n, s_1, s_2, wt = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
        with np.errstate(all="ignore"):
            footprint = (2.0 / w) * g["depth"]
            for qx, qy, wq in taps:
                ok = live & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h)
                qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                r = rec[qy, qx]
                ok = ok & (r[..., 3] > 0.0) & (pk[qy, qx] == g["kind"])
                ndot = dot(g["normal"], pn[qy, qx])
                dist = np.abs(dot(g["normal"], pp[qy, qx] - g["position"])) / footprint
                tests = ok & hit & (wq > TAP_MIN)
                near = np.minimum(np.abs(ndot - normal_min), np.abs(dist - plane_max) / max(1.0, plane_max) if np.isfinite(plane_max) else INF)
                margin = np.minimum(margin, np.where(tests, np.where(np.isnan(near), INF, near), INF))       # a NaN fails on both sides
                ok = ok & (~hit | ((ndot >= normal_min) & (dist <= plane_max)))
                wq = np.where(ok, wq, 0.0)
                e_q = np.where(ok[..., None], r[..., :3], 0.0)
                joined_taps.append((ok, np.where(ok[..., None], r, 0.0)))
                s_e += wq[..., None] * e_q
                s_n += wq * np.where(ok, r[..., 3], 0.0)
                s_1 += wq * np.where(ok, r[..., 4], 0.0)
                s_2 += wq * np.where(ok, r[..., 5], 0.0)
                wt += wq
            usable = wt > 0.01
            den = np.where(usable, wt, 1.0)
            e_r, mu1_r, mu2_r = s_e / den[..., None], s_1 / den, s_2 / den
            n_r = np.minimum(s_n / den, max_history)
            reused = usable & (n_r > 0.0) & finite3(e_cur)
            T1 = n_r + n_cur
            if not identity:
                margin = np.minimum(margin, np.where(live, np.abs(wt - 0.01), INF))
                margin = np.minimum(margin, np.where(reused, np.abs(T1 - 2.0), INF))
            sums = finite(m[..., 0]) & finite(m[..., 1])
            e1 = (n_r[..., None] * e_r + n_cur[..., None] * e_cur) / T1[..., None]
            mu1_1 = (n_r * mu1_r + np.where(sums, m[..., 0], 0.0)) / T1
            mu2_1 = (n_r * mu2_r + np.where(sums, m[..., 1], 0.0)) / T1
            v1 = np.maximum(mu2_1 - mu1_1 ** 2, 0.0) / (T1 - 1.0)
            v1 = np.where((T1 >= 2.0) & finite(mu1_1) & finite(mu2_1) & finite(v1), v1, INF)
            v1 = prepared_variance(v1, g["albedo"], demodulated)
            e = np.where(reused[..., None], e1, e_cur)
            v, T = np.where(reused, v1, v), np.where(reused, T1, n_cur)
            mu1, mu2 = np.where(reused, mu1_1, mu1), np.where(reused, mu2_1, mu2)
            seen = dict(identity=identity, taps=joined_taps, wt=wt, e_r=e_r, n_r=n_r, mu1_r=mu1_r, mu2_r=mu2_r)
    records = np.concatenate([e, np.where(finite3(e), T, 0.0)[..., None], mu1[..., None], mu2[..., None]], -1)
    if watch is not None:
        watch.blended(e=e, v=v, reused=reused, T=T, mu1=mu1, mu2=mu2, seen=seen, scale=lambda plane: prepared_variance(plane, g["albedo"], demodulated))
    e, v, flagged = _passes(e, v, g, b, params.filter.sigma_variance, watch)
    return {"rgb": _finish(e, g["albedo"], demodulated, op), "variance": v, "history": T, "records": records, "reused": reused,
            "pixels_with_history": int(reused.sum()), "margin": margin, "flagged": flagged}
