"""RPT_SHADOW_SEGMENT (rpt.h rpt_set_shadow_mode), the opt-in any-hit walk that leaves out boxes beginning behind the ray's own max_t: a child box is
entered iff the reference's test passes AND tmin <= max_t; the triangle accept test, the root, the ray counts stay the reference's.  Without a GPU:
the ABI carries the mode through every binding; the CPU model of the rule (tools/anyhit_order_sim.cpp sim_any_hit_segment) never GAINS a hit over the
reference's own walk (exact: pruning only removes boxes) and loses none on 10^6 adversarial rays; the bounded walk of real shadow rays is shorter and
finds the same occluders; the `_seg` kernels of the built library hold the occupancy of their exact twins."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_ffi import _p  # noqa: E402
from test_anyhit_order import _shadow_like_rays  # noqa: E402

LIB = os.path.join(ROOT, "rust-path-tracer_amd", "lib", "librpt_hip.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    so = tmp_path_factory.mktemp("segment") / "libanyhit_sim.so"
    subprocess.run(["g++", "-std=c++20", "-O2", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-msse4.1", "-pthread", "-shared", "-o", str(so),
                    os.path.join(ROOT, "tools", "anyhit_order_sim.cpp")], check=True)
    return C.CDLL(str(so))


def test_the_abi_carries_the_mode_through_every_binding(hipmod):
    header = open(os.path.join(ROOT, "include", "rpt", "rpt.h")).read()
    assert re.search(r"enum\s*\{\s*RPT_SHADOW_EXACT\s*=\s*0\s*,\s*RPT_SHADOW_SEGMENT\s*=\s*1\s*\}", header)
    assert re.search(r"int\s+rpt_set_shadow_mode\(rpt_ctx \*ctx, uint32_t mode\);", header)
    assert re.search(r"int\s+rpt_shadow_mode\(rpt_ctx \*ctx, uint32_t \*mode_out\);", header)
    assert re.search(r"int\s+rpt_multi_set_shadow_mode\(rpt_multi \*m, uint32_t mode\);", header)
    assert "#define RPT_ABI_VERSION 3" in header                     # a pure addition
    rust = open(os.path.join(ROOT, "ffi", "rpt.rs")).read()
    for name in ("rpt_set_shadow_mode", "rpt_shadow_mode", "rpt_multi_set_shadow_mode"):
        assert name in hipmod.EXPORTS
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert (hipmod.SHADOW_EXACT, hipmod.SHADOW_SEGMENT) == (0, 1)
    assert "RPT_SHADOW_SEGMENT: u32 = 1" in rust and "RPT_SHADOW_EXACT: u32 = 0" in rust
    for cls in (hipmod.Renderer, hipmod.MultiRenderer):
        assert callable(getattr(cls, "set_shadow_mode"))
    assert callable(hipmod.Renderer.shadow_mode)
    # no environment variable selects the mode: rpt_knobs never change a result
    ctx = open(os.path.join(ROOT, "rust-path-tracer_amd", "csrc", "rpt_ctx.h")).read()
    knobs = ctx[ctx.index("struct rpt_knobs {"):ctx.index("rpt_knobs rpt_read_knobs();")]
    assert "shadow_mode" not in knobs and "SEGMENT" not in knobs


@pytest.mark.parametrize("scene", ["DarkCornell", "VeachMIS", "FurnaceTest", "PBRTest"])
def test_the_bounded_walk_never_gains_a_hit_and_loses_none_of_these(sim, oracle, world, scene):
    """(a) exact: a ray the bounded walk calls occluded is occluded for the reference's walk, in any visiting order.  (b) on these 250 000 rays per scene —
    zero direction components, origins on vertices, max_t at 0.5 / 0.999 / 1 / 1.001 / 2 / 100 x the distance to a point near a vertex — no occlusion is lost
    either: a lost one would be a finding (a triangle with t <= max_t in a box with tmin > max_t), reported with its ray, not a count to allow."""
    w = world(scene)
    sc = oracle.scene(w)
    rng = np.random.default_rng(41)
    n = 250_000
    o, d, max_t = _shadow_like_rays(rng, n, w)
    ref = np.zeros(n, np.uint8)
    sim.sim_any_hit_order(C.byref(sc), C.c_size_t(n), _p(o), _p(d), _p(max_t), 0, C.c_uint32(0), _p(ref))       # intersect_front_to_back<false> itself
    assert 0.02 * n < ref.sum() < 0.98 * n
    for mode, seed in ((0, 0), (1, 0), (3, 0), (4, 1), (4, 2), (5, 0)):   # near / left / far first, random per (ray, node) twice, breadth-first
        got = np.zeros(n, np.uint8)
        sim.sim_any_hit_segment(C.byref(sc), C.c_size_t(n), _p(o), _p(d), _p(max_t), mode, C.c_uint32(seed), _p(got))
        gained = np.flatnonzero((got == 1) & (ref == 0))
        lost = np.flatnonzero((got == 0) & (ref == 1))
        print(f"{scene} mode {mode} seed {seed}: {int(ref.sum())} occluded, gained {len(gained)}, lost {len(lost)}")
        assert len(gained) == 0, (scene, mode, [(o[i].tolist(), d[i].tolist(), float(max_t[i])) for i in gained[:3]])
        assert len(lost) == 0, (scene, mode, len(lost), [(o[i].tolist(), d[i].tolist(), float(max_t[i])) for i in lost[:3]])


def test_rays_without_a_bound_walk_as_before(sim, oracle, world):
    """max_t >= 1e6: the two rules are one walk; a NaN max_t accepts nothing under either"""
    w = world("DarkCornell")
    sc = oracle.scene(w)
    rng = np.random.default_rng(7)
    n = 20_000
    o, d, _ = _shadow_like_rays(rng, n, w)
    for bound in (1e6, 3e6, np.inf, np.nan):
        max_t = np.full(n, bound, np.float32)
        a, b = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        sim.sim_any_hit_order(C.byref(sc), C.c_size_t(n), _p(o), _p(d), _p(max_t), 0, C.c_uint32(0), _p(a))
        sim.sim_any_hit_segment(C.byref(sc), C.c_size_t(n), _p(o), _p(d), _p(max_t), 0, C.c_uint32(0), _p(b))
        assert np.array_equal(a, b), bound
        assert (a.sum() > 0) == (not np.isnan(bound))


def _block_pixels(bx, by):
    return [(by * 8 + y) << 16 | (bx * 8 + x) for y in range(8) for x in range(8)]


@pytest.mark.parametrize("scene,W,H,trips,refill", [("DarkCornell", 1024, 1024, 16, 16), ("VeachMIS", 1920, 1080, 8, 24)])
def test_the_bounded_walk_of_real_shadow_rays_is_shorter(sim, oracle, rpt, world, scene, W, H, trips, refill):
    """The shadow rays the oracle's trace_pixel traces for 64 blocks of 8 x 8 pixels (two samples, bounces 0-3, the rays the device walks), replayed as
    the streamed kernels walk them (sim_wave: trips / refill of the kernel that scene takes): under the segment rule the unoccluded rays visit fewer
    nodes and the same rays are occluded.  No ratio is asserted: profiles/r10_anyhit_sim_segment.txt is the record."""
    w = world(scene)
    sc = oracle.scene(w)
    cfg = rpt.default_config(W, H, nee=1)
    seeds = rpt.blue_noise_seeds(W, H)
    rng = np.random.default_rng(5)
    fields = ["rays", "occluded", "inner_trips", "inner_uniform", "inner_lanes", "leaf_trips", "leaf_iters", "leaf_lanes", "pop_trips", "refills", "skipped", "box_tests", "tri_tests",
              "max_stack", "visits_occluded", "visits_clear", "rays_clear"]                 # SimOut of tools/anyhit_order_sim.cpp
    f = {k: i for i, k in enumerate(fields)}
    total = {0: np.zeros(len(fields), np.float64), 1: np.zeros(len(fields), np.float64)}
    for _ in range(16):                                            # 16 runs of 4 horizontally adjacent blocks
        bx, by = int(rng.integers(0, W // 8 - 4)), int(rng.integers(0, H // 8))
        for bounce in range(4):
            stream = []
            for k in range(4):
                pix = np.array(_block_pixels(bx + k, by), np.uint32)
                for s in range(2):
                    rays = np.zeros((64, 8), np.float32)
                    valid = np.zeros(64, np.uint8)
                    sim.sim_dump_shadow_rays(C.byref(cfg), C.byref(sc), _p(seeds), C.c_uint32(s), C.c_uint32(bounce), _p(pix), C.c_size_t(64), _p(rays), _p(valid))
                    stream.append(rays[valid == 1])
            span = np.ascontiguousarray(np.concatenate(stream))
            if len(span) == 0:
                continue
            hits = {}
            for segment in (0, 1):
                out = np.zeros(24, np.uint64)
                hit = np.zeros(len(span), np.uint8)
                nf = sim.sim_wave_segment(C.byref(sc), _p(span), C.c_uint32(len(span)), 0, trips, refill, _p(out), _p(hit), segment)
                assert nf == len(fields)
                total[segment] += out[:nf].astype(np.float64)
                hits[segment] = hit
            assert np.array_equal(hits[0], hits[1])
    e, s = total[0], total[1]
    print(f"{scene}: {int(e[f['rays']])} rays, {int(e[f['occluded']])} occluded; node visits of an unoccluded ray {e[f['visits_clear']] / e[f['rays_clear']]:.1f} -> "
          f"{s[f['visits_clear']] / s[f['rays_clear']]:.1f}")
    assert e[f["rays"]] == s[f["rays"]] >= 1024                 # (8 192 camera paths: at least one in eight traces a shadow ray the device walks, in the open scene too)
    assert s[f["occluded"]] == e[f["occluded"]] > 0
    assert s[f["rays_clear"]] == e[f["rays_clear"]] > 0
    assert s[f["visits_clear"]] < e[f["visits_clear"]]


# ---- the build: every `_seg` twin of a kernel tests/test_kernel_resources.py names

@pytest.fixture(scope="module")
def resources():
    if not (os.path.exists(LIB) and os.path.exists(OBJDUMP)):
        pytest.skip("librpt_hip.so or the LLVM tools are not here")
    out = subprocess.run([os.path.join(ROOT, "tools", "kernel_resources.sh"), LIB], capture_output=True, text=True, check=True).stdout
    table = {}
    for line in out.splitlines():
        m = re.match(r"\s*(\d+) vgpr\s+(\d+) sgpr\s+(\d+) scratch\s+(\d+) lds\s+(.*)", line)
        if m:
            table.setdefault(m.group(5).strip(), []).append(tuple(int(m.group(k)) for k in (1, 2, 3, 4)))
    return table


VGPR_STEPS = (64, 72, 80, 96, 128, 168, 256, 512)          # 8 / 7 / 6 / 5 / 4 / 3 / 2 / 1 waves per SIMD


def _find(table, prefix):
    hits = [v for k, vs in table.items() if k.startswith(prefix) for v in vs]
    assert hits, prefix
    return hits


@pytest.mark.parametrize("kernel", ["void k_traverse_shadow_stream_seg<16, 1024, false>", "void k_traverse_shadow_stream_seg<16, 1024, true>"])
def test_bounded_lds_walks_fit_two_workgroups_per_cu(resources, kernel):
    for vgpr, sgpr, scratch, lds in _find(resources, kernel):
        assert vgpr <= 64 and sgpr <= 80 and scratch == 0 and lds <= 32 * 1024 + 64


@pytest.mark.parametrize("kernel", ["void k_traverse_shadow_gstream_seg<24, 16, false, false>", "void k_traverse_shadow_gstream_seg<24, 16, false, true>",
                                    "void k_traverse_shadow_gstream_seg<32, 21, false, false>", "void k_traverse_shadow_gstream_seg<32, 21, false, true>"])
def test_bounded_global_walks_keep_eight_waves_per_simd(resources, kernel):
    for vgpr, sgpr, scratch, lds in _find(resources, kernel):
        assert vgpr <= 64 and sgpr <= 80 and scratch == 0


def test_every_shadow_kernel_has_a_bounded_twin_and_none_spills(resources):
    heads = {}                                              # "k_traverse_shadow_gstream<24, 16, false, true>" -> resources (the tool cuts long signatures short)
    for k, vs in resources.items():
        m = re.match(r"void (k_traverse_shadow(?:_stream|_gstream)?(?:_seg)?<[^>]*>)\(", k)
        if m:
            heads[m.group(1)] = vs
    exact = [h for h in heads if "_seg<" not in h]
    assert len(exact) >= 35
    for h in exact:
        twin = h.replace("<", "_seg<", 1)
        assert twin in heads, twin
        for (vgpr, sgpr, scratch, lds), (v0, s0, _, l0) in zip(heads[twin], heads[h]):
            assert scratch == 0 and lds == l0, twin
            # the occupancy of the exact twin: VGPRs are granted in the steps 64 / 72 / 80 / 96 / 128 (tests/test_kernel_resources.py), SGPRs in sixteens
            assert min(x for x in VGPR_STEPS if vgpr <= x) <= min(x for x in VGPR_STEPS if v0 <= x), (twin, vgpr, v0)
            assert -(-sgpr // 16) <= -(-s0 // 16), (twin, sgpr, s0)
    for k in ("void k_traverse_shadow_gstream_seg<32, 16, true, ", "void k_trace_debug_seg<"):
        for vgpr, sgpr, scratch, lds in _find(resources, k):
            assert scratch == 0, k
