"""build_light_pick_table on the GPU (rpt_light_table_build_gpu, csrc/rpt_lights.hip; reference src/light_pick.rs:13-122): the same table —
entries, order, every f32 — as the oracle's sequential restatement (oracle/bvh_oracle.cpp oracle_light_table) and the product's host mirror
(csrc/host/light_table.cpp), on the four shipped scenes, on meshes whose triangles share areas exactly (ties in the stable sort), on a scene
without lights, and with every one of a million triangles emissive."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _inputs(w):
    return np.ascontiguousarray(w.per_vertex["vertex"], np.float32).reshape(-1, 4), w.indices, w.materials


def _same(table, ref_words):
    return np.array_equal(np.ascontiguousarray(table).view(np.uint32).reshape(-1, 7), ref_words)


@pytest.mark.parametrize("scene", ["DarkCornell", "VeachMIS", "FurnaceTest", "PBRTest"])
def test_device_light_table_is_the_sequential_one(hipmod, oracle, world, scene):
    w = world(scene)
    v, t, m = _inputs(w)
    table, n_em, ms = hipmod.light_table_build_gpu(v, t, m)
    ref = oracle.light_table(v, t, m)
    assert _same(table, ref), scene
    assert _same(w.light_pick, ref)                        # what World::from_path built on the host (csrc/host/light_table.cpp) is the same table too
    if scene == "PBRTest":
        assert len(table) == 1 and table["ratio"][0] == -1.0 and n_em == 0
    else:
        assert n_em >= len(table) > 1 and ms["total"] > 0


def test_ties_zero_areas_and_negative_emission(hipmod, oracle):
    """equal probabilities keep index order (stable sort), degenerate emissive triangles get no bin, a material that emits in one channel only"""
    rng = np.random.default_rng(9)
    n = 3000
    from importlib import import_module
    ffi = import_module("rust-path-tracer_amd._ffi")
    base = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    e1 = np.tile(np.array([[1.0, 0, 0], [0.5, 0, 0], [2.0, 0, 0]], np.float32), (n // 3, 1))       # three distinct areas, each shared by 1000 triangles
    e2 = np.tile(np.array([[0, 1.0, 0]], np.float32), (n, 1))
    verts = np.zeros((3 * n, 4), np.float32)
    verts[0::3, :3], verts[1::3, :3], verts[2::3, :3] = base, base + e1, base + e2
    verts[:, 3] = 1.0
    verts[3 * 10 + 2, :3] = verts[3 * 10, :3]               # a degenerate emissive triangle: area 0, probability 0, no bin
    tris = np.zeros(n, ffi.TRIANGLE_DTYPE)
    tris["v0"], tris["v1"], tris["v2"] = np.arange(0, 3 * n, 3), np.arange(1, 3 * n, 3), np.arange(2, 3 * n, 3)
    tris["material"] = rng.integers(0, 4, n)
    mats = np.zeros(4, ffi.MATERIAL_DTYPE)
    mats["emissive"][0, :3] = (3.0, 3.0, 3.0)
    mats["emissive"][1, :3] = (0.0, 0.0, 7.5)
    mats["emissive"][3, :3] = (1.0, 0.25, 0.0)              # material 2 does not emit
    table, n_em, _ = hipmod.light_table_build_gpu(verts, tris, mats)
    ref = oracle.light_table(verts, tris, mats)
    assert _same(table, ref) and len(table) == n_em - (1 if tris["material"][10] != 2 else 0)
    assert np.all(np.diff(table["triangle_pick_pdf_a"]) >= 0)


def test_one_million_emissive_triangles(hipmod, oracle):
    """SURVEY.md 8f N1 at C5 scale: every triangle of the 1 M-triangle scattered stand-in emits (the host builder needs ~240 ms for it)"""
    from scenes import scatter_scene
    w = scatter_scene(1_000_000)
    v, t, _ = _inputs(w)
    mats = w.materials.copy()
    mats["emissive"][:, :3] = np.random.default_rng(1).uniform(0.5, 20.0, (len(mats), 3)).astype(np.float32)
    hipmod.light_table_build_gpu(v[:64], t[:0], mats)      # (first call: code object load)
    best = None
    for _ in range(3):
        table, n_em, ms = hipmod.light_table_build_gpu(v, t, mats)
        best = ms if best is None or ms["total"] < best["total"] else best
    print("light table of", len(table), "entries:", {k: round(x, 2) for k, x in best.items()}, "ms")
    assert n_em == len(t) and len(table) >= n_em - 16
    assert _same(table, oracle.light_table(v, t, mats))
    assert best["total"] < 60.0                             # (30 ms is the target on a quiet box; the bound leaves room for a busy host)


def test_nan_probabilities_are_refused(hipmod, world):
    w = world("DarkCornell")
    v, t, m = _inputs(w)
    v = v.copy()
    v[t["v0"][np.nonzero(np.any(m["emissive"][t["material"], :3] != 0, axis=1))[0][0]], 0] = np.nan
    with pytest.raises(hipmod.RptError, match="NaN"):
        hipmod.light_table_build_gpu(v, t, m)


def test_inputs_without_a_defined_table_are_refused_by_name_never_answered_differently(hipmod, oracle, rpt):
    """Where src/light_pick.rs has no defined answer the device builder must not hand out a table that differs from the sequential one:
    EVERY emissive triangle degenerate -> total power 0 -> every pick probability 0 / 0 = NaN (the reference carries the NaNs through an order-dependent
    sort and a robin-hood loop that never terminates its donor: the sequential builders — host mirror, oracle — reproduce that table, NaN for NaN);
    the device builder refuses the input BY NAME (RPT_ESCENE, "NaN") and the caller keeps the host builder.  A scene whose emissive triangles are only
    PARTLY degenerate is the defined case of test_ties_zero_areas_and_negative_emission."""
    from scenes import textured_scene
    w, _ = textured_scene()
    v, t, m = _inputs(w)
    v = v.copy()
    em = np.nonzero(np.any(m["emissive"][t["material"], :3] != 0, axis=1))[0]
    assert len(em) >= 1
    for k in em:                                            # collapse every emissive triangle onto its first corner
        v[t["v1"][k]] = v[t["v0"][k]]
        v[t["v2"][k]] = v[t["v0"][k]]
    with pytest.raises(hipmod.RptError, match="NaN"):
        hipmod.light_table_build_gpu(v, t, m)
    ht = _host_builder(rpt)(v, t, m)                        # the host mirror through its C entry point: the reference's NaN table, as the oracle restates it
    assert len(ht) == len(t) and np.isnan(ht["ratio"]).all()
    assert _same(ht, oracle.light_table(v, t, m))


def _host_builder(rpt):
    """rpt_light_table_build of librpt_host.so (include/rpt/rpt_host.h) as a function of (vertices, triangles, materials) -> table"""
    from importlib import import_module
    ffi = import_module("rust-path-tracer_amd._ffi")
    L = rpt.host.lib()

    def build(v, t, m):
        out = np.zeros(max(1, len(t)), ffi.LIGHT_PICK_DTYPE)
        n = C.c_size_t(0)
        rc = L.rpt_light_table_build(v.ctypes.data, len(v), np.ascontiguousarray(t).ctypes.data, len(t), np.ascontiguousarray(m).ctypes.data, len(m),
                                     out.ctypes.data, len(out), C.byref(n))
        assert rc == 0
        return out[: n.value]
    return build
