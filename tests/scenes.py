"""Procedural test scenes (data built in Python, run through the reference's BVH / light-table / packing steps)."""
import importlib

import numpy as np


def textured_scene(seed=7):
    """Floor, back wall, a tilted plate with uvs outside [0,1] (wrap), a sphere-ish blob and an area light.
    Materials exercise every texture flag (albedo / metallic / roughness / normal map) of get_pbr_bsdf
    (reference: kernels/src/bsdf.rs:354-387, lib.rs:132-141) through a small RGBA8 atlas."""
    rpt = importlib.import_module("rust-path-tracer_amd")
    rng = np.random.default_rng(seed)
    verts, normals, uvs, tris = [], [], [], []

    def quad(p0, p1, p2, p3, n, mat, uv_scale=1.0, uv_off=0.0):
        b = len(verts)
        verts.extend([p0, p1, p2, p3])
        normals.extend([n] * 4)
        uvs.extend([[uv_off, uv_off], [uv_off + uv_scale, uv_off], [uv_off + uv_scale, uv_off + uv_scale], [uv_off, uv_off + uv_scale]])
        tris.extend([[b, b + 1, b + 2, mat], [b, b + 2, b + 3, mat]])

    quad([-4, 0, -2], [4, 0, -2], [4, 0, 6], [-4, 0, 6], [0, 1, 0], 0)                       # floor
    quad([-4, 0, 6], [4, 0, 6], [4, 5, 6], [-4, 5, 6], [0, 0, -1], 1)                        # back wall
    quad([-2.5, 0.3, 1.5], [-0.5, 0.8, 2.5], [-0.5, 2.2, 2.0], [-2.5, 1.7, 1.0], [0.3, 0.3, -0.9], 2, uv_scale=2.7, uv_off=-0.8)
    quad([0.8, 0.2, 1.0], [2.6, 0.2, 1.8], [2.6, 1.9, 1.8], [0.8, 1.9, 1.0], [0.4, 0.0, -0.9], 3)
    quad([-1, 4.2, 1], [1, 4.2, 1], [1, 4.2, 3], [-1, 4.2, 3], [0, -1, 0], 4)               # light, facing down
    # a coarse blob so the BVH has some depth
    for _ in range(60):
        c = np.array([rng.uniform(-3, 3), rng.uniform(0.2, 2.5), rng.uniform(2.5, 5.5)])
        d = rng.normal(size=(3, 3)) * 0.25
        b = len(verts)
        n = np.cross(d[1] - d[0], d[2] - d[0])
        n = n / np.linalg.norm(n)
        for k in range(3):
            verts.append(list(c + d[k]))
            normals.append(list(n))
            uvs.append([rng.uniform(0, 1), rng.uniform(0, 1)])
        tris.append([b, b + 1, b + 2, int(rng.integers(0, 4))])

    m = np.zeros(5, rpt._ffi.MATERIAL_DTYPE)
    m["albedo"] = [0.8, 0.8, 0.8, 1.0]
    m["roughness"] = 0.6
    m["metallic"] = 0.1
    # atlas rectangles (u0, v0, su, sv) inside a 64x64 atlas: four 32x32 quadrants
    q = {"a": [0.0, 0.0, 0.5, 0.5], "b": [0.5, 0.0, 0.5, 0.5], "c": [0.0, 0.5, 0.5, 0.5], "d": [0.5, 0.5, 0.5, 0.5]}
    m["albedo"][0] = q["a"]; m["has_albedo_texture"][0] = 1
    m["normals"][0] = q["d"]; m["has_normal_texture"][0] = 1
    m["roughness"][0] = q["c"]; m["has_roughness_texture"][0] = 1
    m["metallic"][1] = q["b"]; m["has_metallic_texture"][1] = 1
    m["albedo"][2] = q["a"]; m["has_albedo_texture"][2] = 1
    m["roughness"][2] = 0.15; m["metallic"][2] = 0.9
    m["normals"][3] = q["d"]; m["has_normal_texture"][3] = 1
    m["emissive"][4] = [12.0, 11.0, 9.0, 15.0]
    w = rpt.World.from_buffers(np.array(verts, np.float32), np.array(normals, np.float32), np.array(uvs, np.float32),
                               np.array(tris, np.uint32), m)
    # tangents (only read when a normal texture exists): any unit vector not parallel to the normal
    n = w.per_vertex["normal"][:, :3]
    t = np.cross(n, np.array([0.0, 0.0, 1.0], np.float32))
    bad = np.linalg.norm(t, axis=1) < 1e-3
    t[bad] = np.cross(n[bad], np.array([1.0, 0.0, 0.0], np.float32))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    w.per_vertex["tangent"][:, :3] = t.astype(np.float32)
    atlas = rng.integers(0, 256, (64, 64, 4), dtype=np.uint8)
    atlas[32:, 32:, :2] = rng.integers(96, 160, (32, 32, 2), dtype=np.uint8)     # normal-map quadrant: near +z
    atlas[32:, 32:, 2] = 255
    w.atlas = atlas
    skybox = rng.uniform(0.0, 2.0, (8, 16, 4)).astype(np.float32)
    skybox[..., 3] = 1.0
    return w, skybox


def pbrtest_textured_scene():
    """BASELINE config[3] as it is written — "PBRTest.glb with albedo/normal/rough/metal textures" — on the shipped file, which carries
    NO texture: the file's own buffers (vertices, uvs, BVH, light table) + SYNTHETIC textures, labelled as such.
    Every one of the 26 materials gets the four maps get_pbr_bsdf / the normal-map branch read (bsdf.rs:354-387, lib.rs:132-141), in the
    order World::from_path pushes them (albedo, metallic, roughness, normals: src/asset.rs:138-160), each in the rectangle of the
    4096 x 4096 RGBA8 atlas the reference's own packer gives 104 textures (pack_rects = src/atlas.rs:26-71; uvst = atlas.rs:16-23):
    40 rectangles of 512^2 and 64 of 256^2 texels.  Contents: a two-colour checker with a gradient inside each square (albedo), a rippled
    tangent-space normal, roughness / metallic ramps around the material's own factor.  PBRTest.glb has no TANGENT attribute (the
    reference would get assimp's CalculateTangentSpace, asset.rs:65): tangents are a unit vector perpendicular to the vertex normal."""
    rpt = importlib.import_module("rust-path-tracer_amd")
    w = rpt.World.from_path(rpt.fixture("PBRTest.glb"))
    A = 4096
    n_mat = len(w.materials)
    rects = pack_rects(4 * n_mat, A)
    atlas = np.zeros((A, A, 4), np.uint8)
    atlas[..., 3] = 255
    m = w.materials.copy()

    def uvst(r):
        x, y, rw, rh = r
        return [np.float32(x) / np.float32(A), np.float32(y) / np.float32(A), np.float32(rw) / np.float32(A), np.float32(rh) / np.float32(A)]

    def grid(rw, rh):
        yy, xx = np.mgrid[0:rh, 0:rw].astype(np.float32)
        return xx, yy, xx / np.float32(rw), yy / np.float32(rh)

    def put(r, rgb):
        x, y, rw, rh = r
        atlas[y:y + rh, x:x + rw, :3] = np.clip(np.rint(rgb * 255.0), 0, 255).astype(np.uint8)

    for i in range(n_mat):
        base_rough, base_metal = float(m["roughness"][i][0]), float(m["metallic"][i][0])
        r_alb, r_met, r_rough, r_nrm = rects[4 * i: 4 * i + 4]
        # albedo: checker of 32-texel squares between two colours of the material's own hue, a gradient inside every square
        xx, yy, u, v = grid(r_alb[2], r_alb[3])
        hue = (i * 0.61803398875) % 1.0
        c0 = np.array([0.5 + 0.5 * np.cos(2 * np.pi * (hue + k / 3.0)) for k in range(3)], np.float32) * 0.7 + 0.15
        c1 = 1.0 - 0.6 * c0
        check = ((xx // 32 + yy // 32) % 2)[..., None]
        shade = (0.75 + 0.25 * ((xx % 32) / 32.0))[..., None]
        put(r_alb, (check * c0 + (1 - check) * c1) * shade)
        m["albedo"][i] = uvst(r_alb); m["has_albedo_texture"][i] = 1
        # metallic: vertical ramp around the factor; roughness: horizontal ramp around the factor (the kernels read .x)
        xx, yy, u, v = grid(r_met[2], r_met[3])
        put(r_met, np.repeat(np.clip(base_metal + 0.5 * (v - 0.5), 0.0, 1.0)[..., None], 3, 2))
        m["metallic"][i] = uvst(r_met); m["has_metallic_texture"][i] = 1
        xx, yy, u, v = grid(r_rough[2], r_rough[3])
        put(r_rough, np.repeat(np.clip(base_rough + 0.4 * (u - 0.5), 0.03, 1.0)[..., None], 3, 2))
        m["roughness"][i] = uvst(r_rough); m["has_roughness_texture"][i] = 1
        # normal map: ripples of 64 texels, at most ~17 degrees off +z
        xx, yy, u, v = grid(r_nrm[2], r_nrm[3])
        nx = 0.3 * np.sin(2 * np.pi * xx / 64.0)
        ny = 0.3 * np.cos(2 * np.pi * yy / 48.0)
        nz = np.sqrt(np.maximum(1.0 - nx * nx - ny * ny, 0.0))
        put(r_nrm, np.stack([nx, ny, nz], -1) * 0.5 + 0.5)
        m["normals"][i] = uvst(r_nrm); m["has_normal_texture"][i] = 1
    w.materials = m
    n = w.per_vertex["normal"][:, :3]
    t = np.cross(n, np.array([0.0, 1.0, 0.0], np.float32))
    bad = np.linalg.norm(t, axis=1) < 1e-3
    t[bad] = np.cross(n[bad], np.array([1.0, 0.0, 0.0], np.float32))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    w.per_vertex["tangent"][:, :3] = t.astype(np.float32)
    w.atlas = atlas
    return w


def deep_bvh_scene(n_triangles=200_000, seed=1):
    """Stand-in for the missing BreakTime.glb (BASELINE config 5): clustered long thin triangles
    inside a closed room, a few emissive panels.  Long thin primitives overlap heavily, which makes the binned-SAH
    BVH deep and the traversal divergent."""
    rpt = importlib.import_module("rust-path-tracer_amd")
    rng = np.random.default_rng(seed)
    n_clusters = 64
    centers = np.stack([rng.uniform(-3, 3, n_clusters), rng.uniform(0.3, 4.0, n_clusters), rng.uniform(0.5, 7.0, n_clusters)], 1)
    per = n_triangles // n_clusters
    verts, tris = [], []
    for c in centers:
        base = c + rng.normal(size=(per, 3)) * rng.uniform(0.15, 0.6)
        axis = rng.normal(size=(per, 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        side = np.cross(axis, rng.normal(size=(per, 3)))
        side /= np.linalg.norm(side, axis=1, keepdims=True)
        length = rng.uniform(0.01, 0.12, (per, 1))
        width = rng.uniform(0.002, 0.02, (per, 1))
        v0 = base - axis * length
        v1 = base + axis * length
        v2 = base + side * width
        b = len(verts) * 3
        verts.append(np.stack([v0, v1, v2], 1).reshape(-1, 3))
        idx = b + np.arange(per * 3).reshape(per, 3)
        tris.append(np.concatenate([idx, rng.integers(0, 3, (per, 1))], 1))
    verts = np.concatenate(verts).astype(np.float32)
    tris = np.concatenate(tris).astype(np.uint32)
    # flat normals for the cluster triangles (each owns its 3 vertices)
    p = verts[tris[:, :3].astype(np.int64)]
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
    normals = np.repeat(fn, 3, axis=0).astype(np.float32)
    # closed room (every wall has its own 4 vertices and an INWARD normal, so bounces stay inside) + light panel
    corners = np.array([[-5, 0, -1], [5, 0, -1], [5, 0, 9], [-5, 0, 9], [-5, 6, -1], [5, 6, -1], [5, 6, 9], [-5, 6, 9]], np.float32)
    walls = [((0, 1, 2, 3), (0, 1, 0)), ((7, 6, 5, 4), (0, -1, 0)), ((0, 4, 5, 1), (0, 0, 1)), ((3, 2, 6, 7), (0, 0, -1)),
             ((0, 3, 7, 4), (1, 0, 0)), ((1, 5, 6, 2), (-1, 0, 0))]
    extra_v, extra_n, extra_t = [], [], []
    b = len(verts)
    for q, nrm in walls:
        k = b + len(extra_v)
        extra_v += [corners[i] for i in q]
        extra_n += [nrm] * 4
        extra_t += [[k, k + 1, k + 2, 3], [k, k + 2, k + 3, 3]]
    k = b + len(extra_v)
    extra_v += [[-1.5, 5.9, 2], [1.5, 5.9, 2], [1.5, 5.9, 5], [-1.5, 5.9, 5]]
    extra_n += [(0, -1, 0)] * 4
    extra_t += [[k, k + 2, k + 1, 4], [k, k + 3, k + 2, 4]]        # wound so the geometric normal faces down (emissives are single sided)
    verts = np.concatenate([verts, np.array(extra_v, np.float32)])
    normals = np.concatenate([normals, np.array(extra_n, np.float32)])
    tris = np.concatenate([tris, np.array(extra_t, np.uint32)])
    m = np.zeros(5, rpt._ffi.MATERIAL_DTYPE)
    m["albedo"][:] = [[0.7, 0.2, 0.2, 1], [0.2, 0.7, 0.2, 1], [0.3, 0.3, 0.8, 1], [0.75, 0.75, 0.75, 1], [0, 0, 0, 1]]
    m["roughness"][:, :] = np.array([0.3, 0.6, 0.9, 1.0, 1.0], np.float32)[:, None]
    m["metallic"][:, :] = np.array([0.8, 0.0, 0.3, 0.0, 0.0], np.float32)[:, None]
    m["emissive"][4] = [18.0, 17.0, 15.0, 15.0]
    return rpt.World.from_buffers(verts, normals.astype(np.float32), None, tris, m)


def scatter_scene(n_triangles=60_000, seed=9):
    """Small triangles scattered uniformly in a closed room with a light: the builder splits down to leaves of one or two
    triangles, so the BVH has MORE THAN 65 536 nodes — 32-bit stack entries in the global-memory walks, which no shipped
    scene reaches (PBRTest: 47 637 nodes)."""
    rpt = importlib.import_module("rust-path-tracer_amd")
    rng = np.random.default_rng(seed)
    c = np.stack([rng.uniform(-2.8, 2.8, n_triangles), rng.uniform(0.2, 3.6, n_triangles), rng.uniform(-0.6, 4.6, n_triangles)], 1)
    a = rng.normal(size=(n_triangles, 3)) * 0.03
    b = rng.normal(size=(n_triangles, 3)) * 0.03
    verts = np.stack([c - a, c + a, c + b], 1).reshape(-1, 3).astype(np.float32)
    tris = np.concatenate([np.arange(3 * n_triangles).reshape(-1, 3), rng.integers(0, 2, (n_triangles, 1))], 1).astype(np.uint32)
    p = verts.reshape(-1, 3, 3)
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
    normals = np.repeat(fn, 3, axis=0).astype(np.float32)
    corners = np.array([[-3, 0, -1], [3, 0, -1], [3, 0, 5], [-3, 0, 5], [-3, 4, -1], [3, 4, -1], [3, 4, 5], [-3, 4, 5]], np.float32)
    walls = [((0, 1, 2, 3), (0, 1, 0)), ((7, 6, 5, 4), (0, -1, 0)), ((3, 2, 6, 7), (0, 0, -1)), ((0, 3, 7, 4), (1, 0, 0)), ((1, 5, 6, 2), (-1, 0, 0))]
    ev, en, et = [], [], []
    b0 = len(verts)
    for q, nrm in walls:
        k = b0 + len(ev)
        ev += [corners[i] for i in q]
        en += [nrm] * 4
        et += [[k, k + 1, k + 2, 2], [k, k + 2, k + 3, 2]]
    k = b0 + len(ev)
    ev += [[-1, 3.9, 1], [1, 3.9, 1], [1, 3.9, 3], [-1, 3.9, 3]]
    en += [(0, -1, 0)] * 4
    et += [[k, k + 2, k + 1, 3], [k, k + 3, k + 2, 3]]
    verts = np.concatenate([verts, np.array(ev, np.float32)])
    normals = np.concatenate([normals, np.array(en, np.float32)])
    tris = np.concatenate([tris, np.array(et, np.uint32)])
    m = np.zeros(4, rpt._ffi.MATERIAL_DTYPE)
    m["albedo"][:] = [[0.8, 0.3, 0.2, 1], [0.2, 0.5, 0.8, 1], [0.75, 0.75, 0.75, 1], [0, 0, 0, 1]]
    m["roughness"][:, :] = np.array([0.4, 0.8, 1.0, 1.0], np.float32)[:, None]
    m["metallic"][:, :] = np.array([0.6, 0.0, 0.0, 0.0], np.float32)[:, None]
    m["emissive"][3] = [18.0, 17.0, 15.0, 15.0]
    return rpt.World.from_buffers(verts, normals.astype(np.float32), None, tris, m)


def fat_leaf_scene(n_stack=300, seed=3):
    """A leaf the builder cannot split: n_stack triangles with ONE centroid (rotated copies about it) inside a small room
    with a light.  Every binned-SAH split leaves one side empty, so they stay one leaf of >= 128 triangles: no LDS image
    (leaves of 64+ triangles), several 64-lane rounds of the wave-cooperative leaf test."""
    rpt = importlib.import_module("rust-path-tracer_amd")
    rng = np.random.default_rng(seed)
    c = np.array([0.0, 1.2, 1.5])
    ang = rng.uniform(0, 2 * np.pi, n_stack)
    tilt = rng.uniform(-0.6, 0.6, n_stack)
    r = rng.uniform(0.3, 0.9, n_stack)
    verts, tris = [], []
    for a, t, rad in zip(ang, tilt, r):
        u = np.array([np.cos(a), np.sin(t), np.sin(a)])
        u /= np.linalg.norm(u)
        v = np.cross(u, [0.3, 1.0, 0.2])
        v /= np.linalg.norm(v)
        p0, p1 = c + rad * u, c + rad * (-0.5 * u + 0.866 * v)
        p2 = 3.0 * c - p0 - p1                                    # the third corner makes the centroid exactly (up to rounding) c
        k = len(verts)
        verts += [p0, p1, p2]
        tris.append([k, k + 1, k + 2, int(rng.integers(0, 2))])
    verts = np.array(verts, np.float32)
    p = verts.reshape(-1, 3, 3)
    fn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    fn /= np.maximum(np.linalg.norm(fn, axis=1, keepdims=True), 1e-20)
    normals = np.repeat(fn, 3, axis=0).astype(np.float32)
    corners = np.array([[-3, 0, -1], [3, 0, -1], [3, 0, 5], [-3, 0, 5], [-3, 4, -1], [3, 4, -1], [3, 4, 5], [-3, 4, 5]], np.float32)
    walls = [((0, 1, 2, 3), (0, 1, 0)), ((7, 6, 5, 4), (0, -1, 0)), ((3, 2, 6, 7), (0, 0, -1)), ((0, 3, 7, 4), (1, 0, 0)), ((1, 5, 6, 2), (-1, 0, 0))]
    ev, en, et = [], [], []
    b = len(verts)
    for q, nrm in walls:
        k = b + len(ev)
        ev += [corners[i] for i in q]
        en += [nrm] * 4
        et += [[k, k + 1, k + 2, 2], [k, k + 2, k + 3, 2]]
    k = b + len(ev)
    ev += [[-1, 3.9, 1], [1, 3.9, 1], [1, 3.9, 3], [-1, 3.9, 3]]
    en += [(0, -1, 0)] * 4
    et += [[k, k + 2, k + 1, 3], [k, k + 3, k + 2, 3]]
    verts = np.concatenate([verts, np.array(ev, np.float32)])
    normals = np.concatenate([normals, np.array(en, np.float32)])
    tris = np.concatenate([np.array(tris, np.uint32), np.array(et, np.uint32)])
    m = np.zeros(4, rpt._ffi.MATERIAL_DTYPE)
    m["albedo"][:] = [[0.8, 0.3, 0.2, 1], [0.2, 0.5, 0.8, 1], [0.75, 0.75, 0.75, 1], [0, 0, 0, 1]]
    m["roughness"][:, :] = np.array([0.4, 0.8, 1.0, 1.0], np.float32)[:, None]
    m["metallic"][:, :] = np.array([0.6, 0.0, 0.0, 0.0], np.float32)[:, None]
    m["emissive"][3] = [18.0, 17.0, 15.0, 15.0]
    return rpt.World.from_buffers(verts, normals.astype(np.float32), None, tris, m)


def foreign_pool(w):
    """The same tree as another builder might lay it out: an unused node at index 1, so every child pair sits at (even, odd) — not the (2p + 1, 2p + 2)
    pairs of the reference's builder (src/bvh.rs:296-320: node_count starts at 1).  A valid node buffer of the boundary (children adjacent, links in range)."""
    import copy
    out = copy.copy(w)
    nodes = w.nodes
    new = np.zeros(len(nodes) + 1, nodes.dtype)
    new[0] = nodes[0]
    new[2:] = nodes[1:]
    new[1] = nodes[len(nodes) - 1]                        # (never reached: a copy of some leaf)
    inner = new["triangle_count"] == 0
    inner[1] = False
    new["left_or_first"][inner] += 1
    out.nodes = new
    return out


def write_glb(path, positions, indices, *, normals=None, uvs=None, materials=None, images=None, textures=None, accessor_patch=None,
              node_extra=None):
    """Minimal glTF 2.0 binary writer for tests: one mesh, one primitive, optional embedded PNG images.
    positions (n, 3) float32, indices (m,) uint32.  `accessor_patch(accessors, views)` may corrupt the JSON on purpose."""
    import json
    import struct
    import numpy as np
    blob = bytearray()
    views, accessors = [], []

    def add(data, target=None):
        while len(blob) % 4:
            blob.append(0)
        views.append({"buffer": 0, "byteOffset": len(blob), "byteLength": len(data)})
        blob.extend(data)
        return len(views) - 1

    positions = np.ascontiguousarray(positions, np.float32)
    indices = np.ascontiguousarray(indices, np.uint32)
    attrs = {}
    accessors.append({"bufferView": add(positions.tobytes()), "componentType": 5126, "count": len(positions), "type": "VEC3"})
    attrs["POSITION"] = 0
    if normals is not None:
        accessors.append({"bufferView": add(np.ascontiguousarray(normals, np.float32).tobytes()), "componentType": 5126,
                          "count": len(normals), "type": "VEC3"})
        attrs["NORMAL"] = len(accessors) - 1
    if uvs is not None:
        accessors.append({"bufferView": add(np.ascontiguousarray(uvs, np.float32).tobytes()), "componentType": 5126,
                          "count": len(uvs), "type": "VEC2"})
        attrs["TEXCOORD_0"] = len(accessors) - 1
    accessors.append({"bufferView": add(indices.tobytes()), "componentType": 5125, "count": len(indices), "type": "SCALAR"})
    prim = {"attributes": attrs, "indices": len(accessors) - 1}
    if materials:
        prim["material"] = 0
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0]}], "nodes": [dict({"mesh": 0}, **(node_extra or {}))],
           "meshes": [{"primitives": [prim]}], "accessors": accessors, "bufferViews": views}
    if materials:
        doc["materials"] = materials
    if images:
        doc["images"] = [{"bufferView": add(png), "mimeType": "image/png"} for png in images]
        doc["textures"] = textures if textures is not None else [{"source": i} for i in range(len(images))]
    if accessor_patch:
        accessor_patch(accessors, views)
    doc["buffers"] = [{"byteLength": len(blob)}]
    js = json.dumps(doc).encode()
    js += b" " * (-len(js) % 4)
    while len(blob) % 4:
        blob.append(0)
    total = 12 + 8 + len(js) + 8 + len(blob)
    with open(path, "wb") as f:
        f.write(struct.pack("<III", 0x46546C67, 2, total))
        f.write(struct.pack("<II", len(js), 0x4E4F534A) + js)
        f.write(struct.pack("<II", len(blob), 0x004E4942) + bytes(blob))
    return path


def png_bytes(rgb):
    """Encode an (H, W, 3|4) uint8 array as a PNG (filter 0, zlib level 1) — test input for the loader's decoder."""
    import struct
    import zlib
    import numpy as np
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w, c = rgb.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, w * c)], axis=1).tobytes()

    def chunk(tag, body):
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if c == 3 else 6, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(raw, 1)) + chunk(b"IEND", b""))


def pack_rects(n_textures, atlas=4096):
    """src/atlas.rs:26-71 restated: the leaf rectangle (x, y, w, h) of every texture, in texture order."""
    from collections import deque
    q = deque([(0, 0, atlas, atlas)])
    while len(q) <= n_textures:
        x, y, w, h = q.popleft()
        hw, hh = w // 2, h // 2
        q.extend([(x, y, hw, hh), (x + hw, y, hw, hh), (x, y + hh, hw, hh), (x + hw, y + hh, hw, hh)])
    leafs = sorted(q, key=lambda r: -r[2])          # stable, by width descending
    return leafs[:n_textures]


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# Probe scenes of the float64 second opinion (tests/f64_ref.py): at most eight triangles, built as World objects directly.  The quads of the untextured
# probes reach far outside every view used, and the lamp sits well inside the frame, so that few samples decide anything by a hair.  The textured slab
# is small, so that its uvs vary over the view; its edges and its diagonal are in view.
# ----------------------------------------------------------------------------------------------------------------------------------------------------
PROBE_MATERIALS = {            # name -> (roughness, metallic, albedo); "zero" has an albedo channel of exactly 0
    "r0.5_m0": (0.5, 0.0, (0.8, 0.6, 0.4)), "r1_m0_zero": (1.0, 0.0, (0.7, 0.0, 0.9)), "r0.05_m1": (0.05, 1.0, (0.9, 0.7, 0.5)),
    "r1e-3_m0.5": (1e-3, 0.5, (0.6, 0.8, 0.7)), "r0_m1": (0.0, 1.0, (1.0, 0.8, 0.6))}
PROBE_VIEWS = {                # about 45 degrees onto the slab, and grazing: the camera looks 1 degree below the horizon from a height of 0.25
    "45": dict(cam_position=(0.0, 2.0, 0.0, 0.0), cam_rotation=(0.7853982, 0.0, 0.0, 0.0)),
    "grazing": dict(cam_position=(0.0, 0.25, 0.0, 0.0), cam_rotation=(0.01745329, 0.0, 0.0, 0.0)),
    "corner": dict(cam_position=(0.3, 1.5, -2.0, 0.0), cam_rotation=(0.35, 0.1, 0.0, 0.0)),
    # up into the sky, from 12 to 86 degrees above the horizon: nothing in front
    "up": dict(cam_position=(0.0, 2.0, 0.0, 0.0), cam_rotation=(-0.85, 0.4, 0.0, 0.0))}


def _probe_quad(v, n, t, corners, normal, material):
    k = len(v)
    v += [list(map(float, c)) for c in corners]
    n += [list(map(float, normal))] * 4
    t += [[k, k + 1, k + 2, material], [k, k + 2, k + 3, material]]


def _probe_world(v, n, t, materials):
    rpt = importlib.import_module("rust-path-tracer_amd")
    m = np.zeros(len(materials), rpt._ffi.MATERIAL_DTYPE)
    for i, (roughness, metallic, albedo, emissive) in enumerate(materials):
        m["albedo"][i] = list(albedo) + [1.0]
        m["roughness"][i, :] = roughness
        m["metallic"][i, :] = metallic
        m["emissive"][i] = list(emissive) + [1.0 if any(emissive) else 0.0]
    return rpt.World.from_buffers(np.array(v, np.float32), np.array(n, np.float32), None, np.array(t, np.uint32), m)


_LAMP = (1.0, 0.0, (0.0, 0.0, 0.0), (10.0, 9.0, 8.0))


def probe_slab(material, lamp=False):
    """One quad of 200 x 200 in the plane y = 0, normal up, placed so that its diagonal (the two triangles' common edge) stays outside both views;
    with lamp, ONE emissive triangle 1 above it whose front faces the slab (emitters are single sided: the 45-degree camera, above it, sees its black
    back; the grazing camera, below it, its front)."""
    v, n, t = [], [], []
    roughness, metallic, albedo = PROBE_MATERIALS[material]
    _probe_quad(v, n, t, [(-100, 0, -160), (-100, 0, 40), (100, 0, 40), (100, 0, -160)], (0, 1, 0), 0)
    materials = [(roughness, metallic, albedo, (0.0, 0.0, 0.0))]
    if lamp:
        k = len(v)
        v += [[-0.6, 1.0, 1.4], [0.6, 1.0, 1.4], [0.0, 1.0, 2.4]]
        n += [[0.0, -1.0, 0.0]] * 3
        t += [[k, k + 1, k + 2, 1]]
        materials.append(_LAMP)
    return _probe_world(v, n, t, materials)


def probe_corner():
    """A floor and a wall of two different materials, a lamp above the floor and a small plate between them that shadows part of the floor: seven
    triangles.  Paths bounce between floor and wall; the rest of the sphere is sky."""
    v, n, t = [], [], []
    _probe_quad(v, n, t, [(-60, 0, -60), (-60, 0, 3), (60, 0, 3), (60, 0, -60)], (0, 1, 0), 0)
    _probe_quad(v, n, t, [(-60, 0, 3), (-60, 60, 3), (60, 60, 3), (60, 0, 3)], (0, 0, -1), 1)
    _probe_quad(v, n, t, [(-0.35, 0.9, 1.3), (-0.35, 0.9, 1.9), (0.45, 0.9, 1.9), (0.45, 0.9, 1.3)], (0, 1, 0), 0)
    k = len(v)
    v += [[-0.7, 2.0, 0.9], [0.7, 2.0, 0.9], [0.0, 2.0, 2.2]]
    n += [[0.0, -1.0, 0.0]] * 3
    t += [[k, k + 1, k + 2, 2]]
    return _probe_world(v, n, t, [(0.6, 0.0, (0.7, 0.6, 0.5), (0.0, 0.0, 0.0)), (0.3, 0.8, (0.9, 0.5, 0.3), (0.0, 0.0, 0.0)), _LAMP])


# ---- textured probes --------------------------------------------------------------------------------------------------------------------------------
PROBE_ATLASES = {"32x32": (32, 32), "24x20": (24, 20)}          # (width, height): a power of two, and neither extent one
PROBE_TEXTURE_SETS = {"albedo": ("albedo",), "rough-metal": ("roughness", "metallic"), "normal": ("normals",),
                      "all": ("albedo", "roughness", "metallic", "normals")}
PROBE_SKYBOXES = {"16x8": (16, 8), "7x5": (7, 5)}
# sun_direction of the image-sky probes: only x and z (the rotation about y, atan2(z, x)) and w (the intensity, w / 15) are read.  "zero": no rotation;
# "seam": rotated so that the image's column seam (u = 0 | 1, the direction -x after the rotation) crosses the views
PROBE_SUNS = {"zero": (0.8, 0.6, 0.0, 12.0), "seam": (0.1, 0.3, -0.9, 12.0)}


def probe_atlas(kind):
    """A small asymmetric RGBA8 atlas of four rectangles, one in each quadrant: albedo top left, roughness top right, metallic bottom left, normal map
    bottom right.  A rectangle is its quadrant less the last column and row, so that uv = 1 lands ON the rectangle's last texel and every footprint
    of a uv in [0, 1] stays inside the quadrant (the polyfill sampler has no half-texel offset: a rectangle that fills its quadrant blends its last
    texel with the neighbouring rectangle's first).  Albedo and metallic texels are random, so rows, columns and channels all differ; metallic stays
    below 0.8 in the channel the reference reads (.x; the other channels hold other numbers).  Roughness (.x: 0.39 .. 0.7) and the normal map are ramps
    of a few codes per texel with a pattern on them, never the same in two rows, two columns or two channels; the normal stays near +z, tilted towards
    +x and -y by 4 to 14 degrees.  They are smooth because the float32 error of the interpolated uv, times the map's slope, is an error of the shading
    normal or of the sampled specular direction, which a small cosine between the two amplifies: random texels there would make that error, not a
    misreading, the largest difference (3e-3 to 1e-2 where these give 1e-3).
    -> (atlas (h, w, 4) uint8, {field: (x, y, width, height) in atlas coordinates})"""
    w, h = PROBE_ATLASES[kind]
    rng = np.random.default_rng(w * 100 + h)
    atlas = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    hw, hh = w // 2, h // 2
    atlas[:hh, :hw, :3] = rng.integers(40, 241, (hh, hw, 3))
    row, column = np.mgrid[0:hh, 0:w - hw]
    atlas[:hh, hw:, 0] = 100 + 3 * column + 2 * row + (row * column) % 3
    atlas[hh:, :hw, 0] = rng.integers(0, 201, (h - hh, hw))
    row, column = np.mgrid[0:h - hh, 0:w - hw]
    atlas[hh:, hw:, 0] = 137 + column + (row % 3)
    atlas[hh:, hw:, 1] = 119 - row - 2 * (column % 2)
    atlas[hh:, hw:, 2] = 251 - (row + 2 * column) % 5
    f = np.float32
    rect = lambda x, y, rw, rh: [f(x) / f(w), f(y) / f(h), f(rw - 1) / f(w), f(rh - 1) / f(h)]
    return atlas, {"albedo": rect(0, 0, hw, hh), "roughness": rect(hw, 0, w - hw, hh), "metallic": rect(0, hh, hw, h - hh),
                   "normals": rect(hw, hh, w - hw, h - hh)}


def probe_textured_slab(textures, atlas_kind, uv_range=(0.0, 1.0), lamp=False):
    """One quad of 16 x 16 in the plane y = 0 under the 45-degree view, its uvs running over uv_range in both directions; the material's factors are
    those of "r0.5_m0" where a texture does not replace them.  Tangents: roughly +x, but of lengths 0.7 .. 1.6 and leaning into the normal and
    towards z by amounts that differ from vertex to vertex: the reference normalises only the mapped normal."""
    v, n, t = [], [], []
    _probe_quad(v, n, t, [(-8, 0, -2), (-8, 0, 14), (8, 0, 14), (8, 0, -2)], (0, 1, 0), 0)
    lo, hi = uv_range
    uv_of = lambda p: [lo + (hi - lo) * (p[0] + 8.0) / 16.0, lo + (hi - lo) * (p[2] + 2.0) / 16.0]
    materials = [PROBE_MATERIALS["r0.5_m0"][:2] + (PROBE_MATERIALS["r0.5_m0"][2], (0.0, 0.0, 0.0))]
    if lamp:
        k = len(v)
        v += [[-0.6, 1.0, 1.4], [0.6, 1.0, 1.4], [0.0, 1.0, 2.4]]
        n += [[0.0, -1.0, 0.0]] * 3
        t += [[k, k + 1, k + 2, 1]]
        materials.append(_LAMP)
    rpt = importlib.import_module("rust-path-tracer_amd")
    m = np.zeros(len(materials), rpt._ffi.MATERIAL_DTYPE)
    for i, (roughness, metallic, albedo, emissive) in enumerate(materials):
        m["albedo"][i] = list(albedo) + [1.0]
        m["roughness"][i, :] = roughness
        m["metallic"][i, :] = metallic
        m["emissive"][i] = list(emissive) + [1.0 if any(emissive) else 0.0]
    atlas, rects = probe_atlas(atlas_kind)
    for field in PROBE_TEXTURE_SETS[textures]:
        m[field][0] = rects[field]
        m["has_normal_texture" if field == "normals" else f"has_{field}_texture"][0] = 1
    w = rpt.World.from_buffers(np.array(v, np.float32), np.array(n, np.float32), np.array([uv_of(p) for p in v], np.float32), np.array(t, np.uint32), m)
    p = w.per_vertex["vertex"][:, :3]
    # a function of the position, so that it does not depend on the order the vertices are kept in
    tangent = np.stack([0.7 + 0.9 * (p[:, 2] > 0), 0.25 * np.sign(p[:, 0]) * (p[:, 2] > 0) + 0.1, 0.3 * np.sign(p[:, 0]) - 0.1], 1)
    w.per_vertex["tangent"][:, :3] = tangent.astype(np.float32)
    w.atlas = atlas
    return w


def probe_skybox(case):
    """the float image of an image-sky probe, (h, w, 4) float32 with random texels in 0 .. 2 (rows, columns and channels all differ), or None"""
    kind = PROBE_CASES[case].get("skybox")
    if kind is None:
        return None
    w, h = PROBE_SKYBOXES[kind]
    sky = np.random.default_rng(w * 100 + h).uniform(0.0, 2.0, (h, w, 4)).astype(np.float32)
    sky[..., 3] = 1.0
    return sky


def _textured_probe_cases():
    """the probes behind f64_probes.TEXTURED_TOL and IMAGE_SKY_TOL"""
    cases = {}
    three = dict(min_bounces=3, max_bounces=3)
    # a slab for each texture flag and one with all four; the two atlases alternate, and each is used with all four textures once
    for textures, atlas in (("albedo", "32x32"), ("rough-metal", "24x20"), ("normal", "32x32"), ("all", "24x20")):
        cases[f"tex-{textures}-{atlas}-nee1"] = dict(scene=("tslab", textures, atlas, (0.0, 1.0), True), view="45", config=dict(nee=1, **three), group="textured")
    cases["tex-all-32x32-sky"] = dict(scene=("tslab", "all", "32x32", (0.0, 1.0), False), view="45", config=dict(nee=0, **three), group="textured")
    # the wrap is taken, negative uvs included
    cases["tex-all-24x20-wrap-nee1"] = dict(scene=("tslab", "all", "24x20", (-0.8, 1.9), True), view="45", config=dict(nee=1, **three), group="textured")
    cases["tex-all-32x32-wrap-sky"] = dict(scene=("tslab", "all", "32x32", (-0.8, 1.9), False), view="45", config=dict(nee=0, **three), group="textured")
    # the image sky: every pixel a lookup (both images, both rotations), and bounced rays that reach it from the corner scene
    for sky, sun in (("16x8", "zero"), ("7x5", "seam"), ("16x8", "seam"), ("7x5", "zero")):
        cases[f"imgsky-up-{sky}-{sun}"] = dict(scene=("slab", "r0.5_m0", False), view="up", config=dict(nee=0, **three), skybox=sky, sun=sun, group="image_sky",
                                                   all_sky=True)
    cases["imgsky-corner-16x8-seam-nee1"] = dict(scene=("corner",), view="corner", config=dict(nee=1, min_bounces=0, max_bounces=3), skybox="16x8", sun="seam",
                                                 group="image_sky")
    cases["imgsky-corner-7x5-zero-nee0"] = dict(scene=("corner",), view="corner", config=dict(nee=0, min_bounces=0, max_bounces=5), skybox="7x5", sun="zero",
                                                group="image_sky")
    # (a textured probe by its figure: the slab's lookups, not the sky's, set its difference)
    cases["imgsky-tex-all-24x20-7x5-seam"] = dict(scene=("tslab", "all", "24x20", (-0.8, 1.9), False), view="45", config=dict(nee=0, **three), skybox="7x5",
                                                  sun="seam", group="textured")
    return cases


def _probe_cases():
    cases = {}
    for material in PROBE_MATERIALS:
        for view in ("45", "grazing"):
            cases[f"sky-{material}-{view}"] = dict(scene=("slab", material, False), view=view, config=dict(nee=0, min_bounces=3, max_bounces=3))
    lamp = dict(min_bounces=3, max_bounces=3)
    for nee in (0, 1, 2):
        for view in ("45", "grazing"):
            cases[f"lamp-r0.5_m0-{view}-nee{nee}"] = dict(scene=("slab", "r0.5_m0", True), view=view, config=dict(nee=nee, **lamp))
    for material in list(PROBE_MATERIALS)[1:]:
        cases[f"lamp-{material}-45-nee1"] = dict(scene=("slab", material, True), view="45", config=dict(nee=1, **lamp))
    cases["lamp-r0.5_m0-45-nee1-clamp01"] = dict(scene=("slab", "r0.5_m0", True), view="45", config=dict(nee=1, specular_weight_clamp=(0.0, 1.0), **lamp))
    cases["lamp-r0.5_m0-45-nee1-50x37"] = dict(scene=("slab", "r0.5_m0", True), view="45", config=dict(nee=1, **lamp), size=(50, 37))
    cases["sky-r0.05_m1-45-clamp01"] = dict(scene=("slab", "r0.05_m1", False), view="45",
                                            config=dict(nee=0, min_bounces=3, max_bounces=3, specular_weight_clamp=(0.0, 1.0)))
    cases["sky-r1e-3_m0.5-grazing-50x37"] = dict(scene=("slab", "r1e-3_m0.5", False), view="grazing", config=dict(nee=0, min_bounces=3, max_bounces=3),
                                                 size=(50, 37))
    # Roulette matters where min_bounces < max_bounces - 1: a draw after the last bounce reaches no radiance.  With NEE a bounce takes up to 8 of the
    # sequence's 31 dimensions, so max_bounces = 3 is the longest NEE path the reference's table (and rpt_set_config) allows with min_bounces = 0.
    # Four NEE bounces fit only with min_bounces = 2 (31 dimensions; min_bounces = 1 would need 32): that case covers the full dimension budget and
    # MIS at depth 4, NOT roulette, whose one draw comes after its last bounce.  Roulette with its 1 / prob is covered by corner-nee1-3bounces and
    # by the five-bounce cases, which run without NEE, the lamp found by the BSDF alone.
    cases["corner-nee1-3bounces"] = dict(scene=("corner",), view="corner", config=dict(nee=1, min_bounces=0, max_bounces=3))
    cases["corner-nee1-4bounces-min2"] = dict(scene=("corner",), view="corner", config=dict(nee=1, min_bounces=2, max_bounces=4))
    cases["corner-nee0-5bounces-50x37"] = dict(scene=("corner",), view="corner", config=dict(nee=0, min_bounces=0, max_bounces=5), size=(50, 37))
    cases["corner-nee0-5bounces"] = dict(scene=("corner",), view="corner", config=dict(nee=0, min_bounces=0, max_bounces=5))
    cases.update(_textured_probe_cases())
    return cases


PROBE_CASES = _probe_cases()
PROBE_SIZE, PROBE_SPP = (64, 48), 8


def probe_world(case):
    kind = PROBE_CASES[case]["scene"]
    if kind[0] == "tslab":
        return probe_textured_slab(*kind[1:])
    return probe_corner() if kind[0] == "corner" else probe_slab(kind[1], kind[2])


def probe_config(case):
    rpt = importlib.import_module("rust-path-tracer_amd")
    c = PROBE_CASES[case]
    w, h = c.get("size", PROBE_SIZE)
    sky = dict(has_skybox=1, sun_direction=PROBE_SUNS[c["sun"]]) if "skybox" in c else dict(has_skybox=0)
    return rpt.default_config(w, h, **sky, **PROBE_VIEWS[c["view"]], **c["config"])


# ----------------------------------------------------------------------------------------------------------------------------------------------------
# Inputs of the sampler's function-level tests (tests/test_f64_reference.py on the CPU, tests/test_gpu_sampler.py on the device)
# ----------------------------------------------------------------------------------------------------------------------------------------------------
SAMPLER_EXTENTS = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (64, 64), (63, 65), (64, 48)]         # (width, height)


def sampler_image(width, height, is_u8):
    """(height, width, 4) random texels, every row, column and channel different: uint8 in 64 .. 255, or float32 in 0.5 .. 2.  Texels stay away from
    0 so that the comparison is relative to the value, not to the floor."""
    rng = np.random.default_rng(1000 * width + height + (500 if is_u8 else 0))
    if is_u8:
        return rng.integers(64, 256, (height, width, 4), dtype=np.uint8)
    return rng.uniform(0.5, 2.0, (height, width, 4)).astype(np.float32)


def sampler_coords(width, height):
    """(n, 2) float32, about 26 000: random in [-2, 3]^2; the grid k / extent (where ceil equals floor) over three periods; exactly 0 and 1 and their
    float32 neighbours on both sides; -0.0 and denormals; +-1e10, +-3e38, +-inf and NaN; every special value in either component, against every
    special value and against random ones"""
    f = np.float32
    rng = np.random.default_rng(77 * width + height)
    random = rng.uniform(-2.0, 3.0, (20_000, 2)).astype(f)
    gx = (np.arange(-width, 2 * width + 1, dtype=f) / f(width)).astype(f)
    gy = (np.arange(-height, 2 * height + 1, dtype=f) / f(height)).astype(f)
    grid = np.stack(np.meshgrid(gx, gy, indexing="ij"), -1).reshape(-1, 2)
    grid = grid[rng.permutation(len(grid))[:4000]]
    grid_x = np.stack([rng.choice(gx, 500), rng.uniform(-2.0, 3.0, 500).astype(f)], 1)
    grid_y = np.stack([rng.uniform(-2.0, 3.0, 500).astype(f), rng.choice(gy, 500)], 1)
    zero, one, inf = f(0.0), f(1.0), f(np.inf)
    special = np.array([zero, -zero, one, np.nextafter(zero, one), np.nextafter(zero, -one), np.nextafter(one, zero), np.nextafter(one, f(2.0)),
                        f(1e-45), f(-1e-45), f(1e-40), f(-1e-40), f(1e10), f(-1e10), f(3e38), f(-3e38), inf, -inf, f(np.nan),
                        np.nextafter(f(-1.0), zero), np.nextafter(f(-1.0), f(-2.0)), f(-1.0), f(2.0), np.nextafter(f(2.0), zero)], f)
    pairs = np.stack(np.meshgrid(special, special, indexing="ij"), -1).reshape(-1, 2)
    k = len(special)
    with_random_x = np.stack([np.repeat(special, 12), rng.uniform(-2.0, 3.0, 12 * k).astype(f)], 1)
    with_random_y = np.stack([rng.uniform(-2.0, 3.0, 12 * k).astype(f), np.repeat(special, 12)], 1)
    return np.ascontiguousarray(np.concatenate([random, grid, grid_x, grid_y, pairs, with_random_x, with_random_y]).astype(f))
