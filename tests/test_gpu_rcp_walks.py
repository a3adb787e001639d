"""Tiny scenes that push the triangle test's 1 / det, the rays' 1 / rd, norm3's 1 / len and the roulette's 1 / prob (all rptm::rcp_rn / rcp_rn_window,
csrc/rpt_rcp.h) out of the helper's window and along its edges, where the device returns the division instead of the residual step.  Every image is
held to the CPU oracle bit for bit at 64 x 64, 4 samples, nee 0 and 1; the ray set to the oracle's walk ray by ray.

The window is |x| in [2^-126, 2^126].  What reaches its outside in a render: a determinant of a triangle with edges of 2^63 (the open room scaled by
1.5 x 2^61 and 2^62 about the camera's floor: det = rd . (e1 x e2) = rd.y x 2.25 x 2^126 crosses 2^126 within the image at the first and is inf at the
second: e1 x e2 overflows), the length 0
of an interpolated normal (1 / 0 = inf, 0 x inf = NaN as the reference gives), a roulette probability of inf (a throughput of 1e60 after two bounces
off an albedo of 1e30: the draw is survived and the reciprocal is 0).  A tiny probability (an albedo of 1e-20) is survived by next to no path: that
case holds the draw itself to the reference.  The scales 2^40 and 2^-20 stay inside (a determinant of 2^82; one below the reference's 1e-6
cut, where no reciprocal is taken)."""
import numpy as np
import pytest

import test_gpu_batch_seam as seam

pytestmark = pytest.mark.gpu

W = H = 64
SPP = 4
VIEW = dict(cam_position=(0.0, 1.0, -1.9, 0.0), cam_rotation=(0.45, 0.0, 0.0, 0.0))       # from 1 above the floor, looking down at it
_cache = {}


def room(rpt, scale=1.0, albedo=None, zero_normals=False):
    """Eight triangles: a floor, a back wall and a side wall of a room of 4 x 3 x 4, and a lamp of one quad under where the ceiling would be, scaled
    about the origin — the floor stays in the plane y = 0 under the camera, which is NOT moved, so that its triangles are hit at the same few units of t
    whatever the scale (a hit needs t < 1e6: walls 2^40 away are never accepted, their boxes never entered)."""
    v, n, t = [], [], []
    seam._quad(v, n, t, [(-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2)], (0, 1, 0), 0)
    seam._quad(v, n, t, [(-2, 0, 2), (-2, 3, 2), (2, 3, 2), (2, 0, 2)], (0, 0, -1), 1)
    seam._quad(v, n, t, [(-2, 0, -2), (-2, 3, -2), (-2, 3, 2), (-2, 0, 2)], (1, 0, 0), 2)
    seam._quad(v, n, t, [(-0.5, 2.9, -0.5), (0.5, 2.9, -0.5), (0.5, 2.9, 0.5), (-0.5, 2.9, 0.5)], (0, -1, 0), 3)
    m = seam._materials(rpt, [12.0, 11.0, 9.0, 1.0])
    if albedo is not None:
        m["albedo"][:3] = albedo
    w = rpt.World.from_buffers(np.array(v, np.float32) * np.float32(scale), np.array(n, np.float32), None, np.array(t, np.uint32), m)
    if zero_normals:
        # the floor's vertex normals (0, 1, 0), (0, -1, 0) in turn: the interpolated normal passes through 0 along a line of every triangle, and IS 0
        # wherever the weights of the two kinds are equal floats
        nrm = w.per_vertex["normal"]
        floor = nrm[:, 1] == 1.0
        assert floor.sum() == 4
        nrm[np.flatnonzero(floor)[::2], :3] = (0.0, -1.0, 0.0)
    return w


CASES = {
    "scaled 2^40": lambda rpt: room(rpt, 2.0 ** 40),
    "scaled 2^-20": lambda rpt: room(rpt, 2.0 ** -20),
    "scaled 1.5 x 2^61": lambda rpt: room(rpt, 1.5 * 2.0 ** 61),
    "scaled 2^62": lambda rpt: room(rpt, 2.0 ** 62),
    "zero normal": lambda rpt: room(rpt, zero_normals=True),
    "tiny roulette probability": lambda rpt: room(rpt, albedo=[1e-20, 1e-20, 1e-20, 1.0]),
    "huge roulette probability": lambda rpt: room(rpt, albedo=[1e30, 1e30, 1e30, 1.0]),
}


def the_case(rpt, oracle, case, nee):
    """(world, config, seeds, the oracle's result): computed once, never changed"""
    if (case, nee) not in _cache:
        if case not in _cache:
            _cache[case] = CASES[case](rpt)
        w = _cache[case]
        # min_bounces 0: the roulette is played from the second bounce on
        cfg = rpt.default_config(W, H, nee=nee, min_bounces=0, max_bounces=4 if nee == 0 else 3, **VIEW)
        seeds = rpt.blue_noise_seeds(W, H)
        acc, _, st = oracle.trace_cpu(cfg, oracle.scene(w), seeds, SPP)
        acc.setflags(write=False)
        _cache[(case, nee)] = (w, cfg, seeds, acc, st)
    return _cache[(case, nee)]


def floor_determinant_straight_down(w):
    """|det| of the triangle test for the direction (0, -1, 0) on the floor's first triangle: |(e1 x e2).y|"""
    p = w.per_vertex["vertex"][:, :3].astype(np.float64)
    floor = np.flatnonzero((w.per_vertex["normal"][:, 1] == 1.0) & (p[:, 1] == 0))
    assert floor.size == 4
    i0, i1, i2 = floor[:3]
    return abs(float(np.cross(p[i1] - p[i0], p[i2] - p[i0])[1]))


@pytest.mark.parametrize("nee", [0, 1])
@pytest.mark.parametrize("case", sorted(CASES))
def test_image_equals_the_oracle_bit_for_bit(hipmod, oracle, rpt, case, nee):
    w, cfg, seeds, acc_c, st_c = the_case(rpt, oracle, case, nee)
    acc, st, _, _ = seam._render(hipmod, w, cfg, seeds, (SPP,))
    print(f"{case}, nee {nee}: {st_c.extension_rays} extension rays, {st_c.shadow_rays} shadow rays, {st_c.sky_evals} sky evaluations; "
          f"{int(np.isnan(acc_c).any(axis=2).sum())} pixels hold a NaN")
    assert st["extension_rays"] == st_c.extension_rays and st["sky_evals"] == st_c.sky_evals and st["shadow_rays"] == st_c.shadow_rays
    differ = acc.view(np.uint32) != acc_c.view(np.uint32)
    assert not differ.any(), f"{int(differ.sum())} accumulator words differ"
    # fit for the purpose (from the oracle alone)
    if case in ("scaled 2^40", "scaled 1.5 x 2^61", "zero normal", "tiny roulette probability", "huge roulette probability"):
        assert st_c.extension_rays > W * H * SPP * 1.2                # the floor is hit: paths go on
    if case in ("scaled 2^-20", "scaled 2^62"):
        assert st_c.extension_rays == W * H * SPP                    # every determinant below the cut, resp. inf (its reciprocal 0): nothing is hit
    if case == "huge roulette probability":
        assert np.isnan(acc_c).any()                                  # a probability of inf is survived, inf x (1 / inf) = NaN
    if case == "zero normal":
        assert np.isnan(acc_c).any()                                  # 0 x inf reached the image, as in the reference


def test_the_scaled_rooms_put_the_determinant_where_they_should(rpt):
    det = {s: floor_determinant_straight_down(room(rpt, 2.0 ** s)) for s in (40, -20, 62)}
    det[61.5] = floor_determinant_straight_down(room(rpt, 1.5 * 2.0 ** 61))
    assert 1e-6 < det[40] < 2.0 ** 126 and det[-20] < 1e-6
    assert det[61.5] == 2.25 * 2.0 ** 126                # times |rd.y|, which the view spreads from about 0.1 to 0.8: determinants on both sides of 2^126
    assert det[62] >= 2.0 ** 128                                                        # inf in float32


def edge_rays(w, n_each=64):
    """rays into DarkCornell whose direction components sit on both sides of fastdiv_divisor_ok's bounds (|y| in [2^-40, 4): below 2^-40, at it, the
    last float below 4, at 4) in every component in turn, the other two random — the rays' reciprocals are taken by rcp_rn_window inside the bounds and
    not at all outside"""
    rng = np.random.default_rng(20)
    f = np.float32
    edges = np.array([f(2.0 ** -40), np.nextafter(f(2.0 ** -40), f(0)), np.nextafter(f(2.0 ** -40), f(1)), f(4.0), np.nextafter(f(4.0), f(0)),
                      np.nextafter(f(4.0), f(8)), f(2.0 ** -41), f(2.0 ** -126), f(0.0)], f)
    lo = w.per_vertex["vertex"][:, :3].min(axis=0)
    hi = w.per_vertex["vertex"][:, :3].max(axis=0)
    o, d = [], []
    for axis in range(3):
        for e in edges:
            for sign in (1.0, -1.0):
                dd = rng.normal(size=(n_each, 3)).astype(f)
                dd[:, axis] = f(sign) * e
                d.append(dd)
                o.append((lo + rng.random((n_each, 3)) * (hi - lo)).astype(f))
    return np.concatenate(o), np.concatenate(d)


def test_rays_at_the_edges_of_the_divisor_guard(hipmod, oracle, rpt, world):
    w = world("DarkCornell")
    renderer = hipmod.Renderer(0)
    try:
        _edge_rays_against_the_oracle(renderer, oracle, rpt, w)
    finally:
        renderer.close()


def _edge_rays_against_the_oracle(renderer, oracle, rpt, w):
    sc = oracle.scene(w)
    o, d = edge_rays(w)
    renderer.upload_scene(w)
    t_c, tri_c, fl_c, err = oracle.trace_rays(sc, 0, o, d)
    assert err == 0
    hit = (fl_c & 1) == 1
    assert hit.sum() > len(o) // 2
    t_g, tri_g, fl_g = renderer.debug_trace_rays(False, o, d)
    assert np.array_equal(fl_g, fl_c) and np.array_equal(t_g.view(np.uint32), t_c.view(np.uint32)) and np.array_equal(tri_g[hit], tri_c[hit])
    max_t = (np.random.default_rng(21).random(len(o)) * 4).astype(np.float32)
    _, _, afl_g = renderer.debug_trace_rays(True, o, d, max_t)
    _, _, afl_c, err = oracle.trace_rays(sc, 1, o, d, max_t)
    assert err == 0 and np.array_equal(afl_g & 1, afl_c & 1)
    # the production stage (the streamed LDS walk for this scene)
    renderer.set_config(rpt.default_config(128, 128))
    renderer.reset(rpt.blue_noise_seeds(128, 128))
    t_p, tri_p, fl_p = renderer.debug_trace_rays_production(o, d)
    renderer.reset(rpt.blue_noise_seeds(128, 128))
    assert np.array_equal(fl_p, fl_c) and np.array_equal(t_p.view(np.uint32), t_c.view(np.uint32)) and np.array_equal(tri_p[hit], tri_c[hit])
