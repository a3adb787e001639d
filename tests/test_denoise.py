"""The denoiser without a GPU: the host build of csrc/k_denoise.h (hipmod.denoise_host) against the numpy restatement of tests/denoise_ref.py, bit for bit;
the properties the filter must have; and its quality against converged oracle images of the shipped scenes."""
import os

import numpy as np
import pytest

import denoise_ref
from conftest import ROOT, rel_l2

SIZES = [(1, 1), (70, 9), (130, 200)]                 # (width, height)


def synthetic_guides(w, h, seed):
    """guide buffers with every kind, patches of equal kind (so that taps do join), tilted normals, albedos on both sides of the 0.01 floor"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    kind = ((xs // 5 + ys // 3 + rng.integers(0, 2, (h, w)) * (rng.random((h, w)) < 0.1)) % 3).astype(np.uint32)
    normal = rng.normal(size=(h, w, 3)).astype(np.float32) * 0.2 + np.array([0.0, 0.3, -1.0], np.float32)
    normal = (normal / np.linalg.norm(normal, axis=-1, keepdims=True)).astype(np.float32)
    normal[kind == 0] = 0.0
    normal[rng.random((h, w)) < 0.02] = 0.0                                    # a hit whose normal normalised to nothing
    depth = (3.0 + 0.01 * xs + 0.02 * ys + rng.random((h, w)) * 0.05).astype(np.float32)
    depth[kind == 0] = 1e6
    position = (np.stack([xs * 0.01, ys * 0.01, np.zeros_like(xs, float)], -1) * depth[..., None]).astype(np.float32)
    albedo = rng.choice(np.array([0.0, 0.004, 0.01, 0.2, 0.8, 1.0], np.float32), (h, w, 3))
    albedo[kind != 1] = 1.0
    return {"albedo": albedo, "normal": normal, "position": position, "depth": depth, "kind": kind}


def noisy_image(w, h, seed):
    rng = np.random.default_rng(seed + 100)
    return (rng.gamma(2.0, 0.3, (h, w, 3))).astype(np.float32)


def assert_same_bits(got, want, what):
    ng, nw = np.isnan(got), np.isnan(want)
    assert np.array_equal(ng, nw), what
    assert np.array_equal(got[~ng].view(np.uint32), want[~nw].view(np.uint32)), f"{what}: {np.count_nonzero(got[~ng].view(np.uint32) != want[~nw].view(np.uint32))} words differ"


@pytest.mark.parametrize("w,h", SIZES)
def test_host_filter_equals_the_numpy_restatement_bitwise(hipmod, oracle, w, h):
    """every iteration count 0..6 with demodulation on and off (the tonemap operator cycling), every operator at 3 iterations, and sigma_color = 0"""
    g, img = synthetic_guides(w, h, w * 1000 + h), noisy_image(w, h, w)
    cases = [(it, dem, (it + dem) % 7, 1.5, 1.0, 2) for it in range(7) for dem in (0, 1)]
    cases += [(3, 1, op, 0.8, 2.0, 5) for op in range(7)]
    cases += [(4, 1, 0, 0.0, 1.0, 0), (2, 0, 3, 0.0, 0.5, 10), (6, 1, 4, 3.0, 0.0, 3)]
    for it, dem, op, sc, sp, npl in cases:
        p = hipmod.denoise_params(iterations=it, demodulate=dem, sigma_color=sc, sigma_plane=sp, normal_power_log2=npl)
        got = hipmod.denoise_host(img, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], p, op)
        want = denoise_ref.denoise(img, g, p, op, oracle)
        assert_same_bits(got, want, f"{w}x{h} iterations {it} demodulate {dem} op {op} sigma_color {sc} sigma_plane {sp} normal_power_log2 {npl}")


@pytest.mark.parametrize("w,h", SIZES)
def test_host_filter_on_hostile_images(hipmod, oracle, w, h):
    """images holding NaN, infinities, negative, huge, denormal and zero values: host == numpy, NaN for NaN, for every operator"""
    rng = np.random.default_rng(8 + w)
    vals = np.array([0.0, -0.0, 1.0, 0.18, 1e-42, 1e-30, 1e30, 3e38, -1.0, -1e30, np.nan, np.inf, -np.inf, 7.5, 0.999], np.float32)
    g = synthetic_guides(w, h, 5)
    img = vals[rng.integers(0, len(vals), (h, w, 3))].copy()
    tame = rng.random((h, w)) < 0.6                                           # most pixels ordinary: hostile values meet finite neighbours
    img[tame] = noisy_image(w, h, 3)[tame]
    for op in range(7):
        for dem in (0, 1):
            p = hipmod.denoise_params(iterations=3, demodulate=dem)
            got = hipmod.denoise_host(img, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], p, op)
            assert_same_bits(got, denoise_ref.denoise(img, g, p, op, oracle), f"{w}x{h} op {op} demodulate {dem}")
    # guides that are themselves degenerate (infinite positions, zero depth): no NaN may enter a finite pixel's sum
    g["position"][rng.random((h, w)) < 0.1] = np.inf
    g["depth"][rng.random((h, w)) < 0.1] = 0.0
    clean = noisy_image(w, h, 4)
    p = hipmod.denoise_params(iterations=4)
    got = hipmod.denoise_host(clean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], p, 0)
    assert np.isfinite(got).all()
    assert_same_bits(got, denoise_ref.denoise(clean, g, p, 0, oracle), "degenerate guides")


def test_zero_iterations_is_resolve(hipmod, oracle):
    """iterations = 0 skips demodulation altogether: the result is oracle.resolve of the same sums, bit for bit, for every operator"""
    w, h = 70, 9
    g = synthetic_guides(w, h, 1)
    acc = np.zeros((h, w, 4), np.float32)
    acc[..., :3] = noisy_image(w, h, 2) * 7.0
    acc[..., 3] = 7.0
    mean = (acc[..., :3] / np.float32(7.0)).astype(np.float32)
    for op in range(7):
        got = hipmod.denoise_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], hipmod.denoise_params(iterations=0, demodulate=1), op)
        assert_same_bits(got, oracle.resolve(acc, 7.0, op), f"op {op}")


def test_parameter_checks(hipmod):
    g, img = synthetic_guides(8, 8, 1), noisy_image(8, 8, 1)
    run = lambda p, op=0: hipmod.denoise_host(img, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], p, op)
    run(hipmod.denoise_params(iterations=6, normal_power_log2=10))
    for bad in (dict(iterations=7), dict(normal_power_log2=11), dict(sigma_color=-1.0), dict(sigma_plane=float("nan")), dict(sigma_color=float("inf"))):
        with pytest.raises(hipmod.RptError) as e:
            run(hipmod.denoise_params(**bad))
        assert e.value.code == -1, bad
    with pytest.raises(hipmod.RptError):
        run(hipmod.denoise_params(), op=7)
    d = hipmod.denoise_params()
    assert 1 <= d.iterations <= 6 and d.normal_power_log2 <= 10 and d.sigma_color >= 0 and d.sigma_plane > 0 and d.demodulate in (0, 1)


def furnace(rpt, world, oracle, spp=4, size=256):
    cfg = rpt.default_config(size, size, nee=0)                              # the reference's furnace test (tests/correctness_tests.rs:14-33), at twice its size
    w = world("FurnaceTest")
    acc, _, _ = oracle.trace_cpu(cfg, oracle.scene(w), rpt.blue_noise_seeds(size, size), spp)
    return (acc[..., :3] / np.float32(spp)).astype(np.float32), denoise_ref.guides(w, cfg, oracle)


def reached(seed, member, passes):
    """the pixels of `member` whose value after `passes` a-trous passes can depend on a pixel of `seed`: pass i joins taps at offsets 2^i (dx, dy), dx, dy in -2..2"""
    r = seed & member
    for i in range(passes):
        s, grown = 1 << i, r.copy()
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                shifted = np.zeros_like(r)
                ys, xs = slice(max(0, dy * s), r.shape[0] + min(0, dy * s)), slice(max(0, dx * s), r.shape[1] + min(0, dx * s))
                yd, xd = slice(max(0, -dy * s), r.shape[0] + min(0, -dy * s)), slice(max(0, -dx * s), r.shape[1] + min(0, -dx * s))
                shifted[yd, xd] = r[ys, xs]
                grown |= shifted
        r = grown & member
    return r


def test_furnace_stays_constant(rpt, hipmod, world, oracle):
    """What is constant in a furnace stays constant: sum(w c) / sum(w) = c up to rounding.  Bound: 5 passes x 26 roundings (25 additions into each sum and the
    division) x 2^-24, relative.  Two readings, both held:
    (a) the oracle's 4-spp render of FurnaceTest.glb with the reference's furnace configuration.  The emitter all around (kind 2) is rendered as exactly its
        emission, except at the sphere's silhouette, where a jittered sample of a pixel whose centre ray sees the emitter can land on the sphere.  Only pixels of
        one kind ever join a sum, so every emitter pixel that no silhouette pixel can reach through the taps of five passes must come back as the emission;
        the noisy sphere beside it is filtered meanwhile.  (At 256 x 256 — twice the reference's size — that is the outer band of the image.)
        The emitter pixels within its reach are not constant in the INPUT (their 4 samples include sphere hits), so they cannot come back constant; they stay
        within the range of the emitter pixels that feed them, which is asserted too.
    (b) the furnace's converged image, a constant, over the same guides: every pixel."""
    bound = 5 * 26 * 2.0 ** -24
    mean, g = furnace(rpt, world, oracle)
    emitter = g["kind"] == 2
    assert emitter.sum() > 1000 and (g["kind"] == 1).sum() > 100
    value = mean[0, 0]
    assert np.all(value > 0) and g["kind"][0, 0] == 2
    clean = emitter & ~reached(emitter & (mean != value).any(axis=-1), emitter, 5)
    print(f"furnace: {emitter.sum()} emitter pixels, {clean.sum()} out of the silhouette's reach")
    assert clean.sum() > 10000 and np.all(mean[clean] == value)
    for dem in (0, 1):
        p = hipmod.denoise_params(iterations=5, demodulate=dem)
        out = hipmod.denoise_host(mean, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], p, 0)
        rel = np.abs(out[clean].astype(np.float64) - value) / value
        print(f"furnace emitter region, demodulate {dem}: max relative deviation {rel.max():.3e} (bound {bound:.3e})")
        assert rel.max() <= bound
        # the emitter pixels within the silhouette's reach are means of emitter pixels only (no sphere pixel joins them): within the range of those inputs
        lo, hi = mean[emitter].min(axis=0).astype(np.float64), mean[emitter].max(axis=0).astype(np.float64)
        near = out[emitter & ~clean].astype(np.float64)
        assert len(near) > 100 and np.all(near >= lo * (1 - bound)) and np.all(near <= hi * (1 + bound))
        sphere = g["kind"] == 1
        assert (out[sphere] != mean[sphere]).any(axis=-1).mean() > 0.5                # (the noisy sphere is filtered)
        const = np.full_like(mean, 0.5994)                                    # 0.8^2.2, the value the reference's furnace assertion expects
        out = hipmod.denoise_host(const, np.ones_like(g["albedo"]), g["normal"], g["position"], g["depth"], g["kind"], p, 0)
        rel = np.abs(out.astype(np.float64) - const) / const
        print(f"constant image over the furnace guides, demodulate {dem}: max relative deviation {rel.max():.3e}")
        assert rel.max() <= bound


def test_a_pixel_alone_in_its_kind_comes_back_unchanged(hipmod):
    """a pixel whose 24 neighbours all have another kind: no tap joins it.  Without demodulation it comes back bit for bit; with it, the value makes the round
    trip c / a * a, two roundings (2^-23 relative)."""
    w, h = 9, 7
    g, img = synthetic_guides(w, h, 3), noisy_image(w, h, 9)
    g["kind"][:] = 1
    g["kind"][3, 4] = 2
    g["albedo"][3, 4] = [0.3, 0.6, 0.9]
    out = hipmod.denoise_host(img, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], hipmod.denoise_params(iterations=1, demodulate=0), 0)
    assert np.array_equal(out[3, 4].view(np.uint32), img[3, 4].view(np.uint32))
    assert (out != img).any(axis=-1).sum() > w * h // 2                      # (its neighbours are filtered)
    out = hipmod.denoise_host(img, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], hipmod.denoise_params(iterations=1, demodulate=1), 0)
    assert np.all(np.abs(out[3, 4].astype(np.float64) - img[3, 4]) <= 2.0 ** -23 * img[3, 4])


def test_the_filter_reduces_the_error_against_converged_images(rpt, hipmod, world, oracle):
    """On DarkCornell (nee 0), VeachMIS (nee 1) and PBRTest (nee 0) at 128 x 128: the oracle's 8-spp mean, denoised with the default parameters over the numpy
    guides, is closer (rel-L2) to the oracle's 1024-spp mean than the 8-spp mean itself.  The ratios are kept in profiles/r11_denoise_quality.txt
    (tools/denoise_probe.py --quality rewrites the file, grid included)."""
    for scene, nee in denoise_ref.QUALITY:
        noisy, conv, g = denoise_ref.quality_images(rpt, world, oracle, scene, nee)
        den = hipmod.denoise_host(noisy, g["albedo"], g["normal"], g["position"], g["depth"], g["kind"], None, 0)
        e_noisy, e_den = rel_l2(noisy, conv), rel_l2(den, conv)
        print(f"{scene} nee {nee}: rel-L2 noisy {e_noisy:.4f} denoised {e_den:.4f} ratio {e_den / e_noisy:.3f}")
        assert np.isfinite(den).all()
        assert e_den < e_noisy, (scene, e_den, e_noisy)


def test_quality_record_is_kept():
    text = open(os.path.join(ROOT, "profiles", "r11_denoise_quality.txt")).read()
    assert all(s in text for s in ("DarkCornell", "VeachMIS", "PBRTest")) and "grid" in text
