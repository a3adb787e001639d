/*
 * rpt_scene.hip — scene preparation of librpt_hip.so: validation of the uploaded buffers (host and device), the derived
 * per-triangle records, the LDS image and the pair records of the streamed walks, the order probes of shadow_order.h as
 * kernels, and rpt_upload_scene, which runs them as a sequence of steps.
 */
#include <algorithm>
#include <cstring>

#include "rpt_ctx.h"             /* (brings shadow_order.h) */
#include "rpt_fastdiv.h"

namespace {

/* what needs no walk: sizes, and every index of the triangle and light-pick buffers in range */
int validate_scene_flat(rpt_ctx *ctx, const rpt_per_vertex_data *pv, size_t nv, const rpt_triangle *idx, size_t nt, size_t nn, const rpt_material_data *mats, size_t nm,
                        const rpt_light_pick_entry *lp, size_t nlp) {
    (void)pv; (void)mats;
    if (!nv || !nt || !nn || !nm || !nlp) { ctx->error = "empty scene buffer"; return RPT_ESCENE; }
    if (nt >= 0x7ffffff0ull || nn >= 0x7ffffff0ull) { ctx->error = "scene too large for 31-bit indices"; return RPT_ESCENE; }
    for (size_t i = 0; i < nt; ++i)
        if (idx[i].v0 >= nv || idx[i].v1 >= nv || idx[i].v2 >= nv || idx[i].material >= nm) {
            ctx->error = "index buffer entry out of range";
            return RPT_ESCENE;
        }
    bool sentinel = lp[0].ratio < 0.0f;
    if (!sentinel)
        for (size_t i = 0; i < nlp; ++i)
            if (lp[i].triangle_index_a >= nt || lp[i].triangle_index_b >= nt) {
                ctx->error = "light pick entry out of range";
                return RPT_ESCENE;
            }
    return RPT_OK;
}

/* The whole validation on the host (the debug hooks, which have no device): the flat part + the node pool as a TREE — children in range, no node reached twice
 * (a cycle, or a subtree with two parents), leaf ranges inside the index buffer, depth bounded.  rpt_upload_scene checks the tree on the device (device_validate_tree:
 * the same four conditions, level by level; the DFS over the 2 M nodes of the scattered stand-in was 16 - 20 ms of its upload). */
int validate_scene(rpt_ctx *ctx, const rpt_per_vertex_data *pv, size_t nv, const rpt_triangle *idx, size_t nt,
                   const rpt_bvh_node *nodes, size_t nn, const rpt_material_data *mats, size_t nm,
                   const rpt_light_pick_entry *lp, size_t nlp, uint32_t &max_depth) {
    RPT_TRY(validate_scene_flat(ctx, pv, nv, idx, nt, nn, mats, nm, lp, nlp));
    std::vector<std::pair<uint32_t, uint32_t>> stack{{0u, 0u}};
    std::vector<bool> seen(nn, false);
    max_depth = 0;
    while (!stack.empty()) {
        auto [n, d] = stack.back();
        stack.pop_back();
        if (seen[n]) { ctx->error = "BVH is not a tree"; return RPT_ESCENE; }
        seen[n] = true;
        if (d > max_depth) max_depth = d;
        const rpt_bvh_node &node = nodes[n];
        if (node.triangle_count > 0) {
            if ((size_t)node.left_or_first + node.triangle_count > nt) { ctx->error = "BVH leaf range out of bounds"; return RPT_ESCENE; }
        } else {
            if ((size_t)node.left_or_first + 1 >= nn) { ctx->error = "BVH child index out of bounds"; return RPT_ESCENE; }
            stack.push_back({node.left_or_first, d + 1});
            stack.push_back({node.left_or_first + 1, d + 1});
        }
    }
    if (max_depth > 31) {   /* reference: FixedVec<usize, 32> would overflow (intersection.rs:178) */
        ctx->error = "BVH deeper than the reference's 32-entry traversal stack";
        return RPT_ESCENE;
    }
    return RPT_OK;
}

/* The LDS-resident traversal image of a small scene (layout and rationale: k_walk.h, SceneViewLds):
 *   float4 K_A[P], K_B[P] for K = x, y, z   (L.lo, R.lo, L.hi, R.hi) and (L.hi, R.hi, L.lo, R.lo)
 *   u32    D[P] (padded to 16 bytes)        desc(L) | desc(R) << 16
 *   float4 (a, e1, e2)[T]
 * with pair p = nodes (2p+1, 2p+2).  Returns false when the node array cannot be represented (not pair-shaped,
 * a box with lo > hi or a NaN bound, a leaf of 64+ triangles, 512+ triangles): such a scene is traversed from
 * global memory by the generic loop. */
bool build_lds_image(const rpt_bvh_node *nodes, size_t nn, const std::vector<float4> &geom, size_t nt,
                     std::vector<float4> &image, uint32_t &pairs, uint32_t &root) {
    if (nn == 0 || (nn & 1u) == 0u || nt > 512 || 2 * nn >= (size_t)LDS_DESC_DEAD) return false;      /* (4 x pair index < LDS_DESC_DEAD) */
    auto desc = [&](const rpt_bvh_node &n, uint32_t &out) {
        if (n.triangle_count != 0u) {
            if (n.triangle_count >= 64u || n.left_or_first >= 512u || (size_t)n.left_or_first + n.triangle_count > nt) return false;
            /* what the streamed walks rely on where they keep the REST of a leaf as a descriptor (k_walk.h lds_stream_walk_run ONE_TRI): every (first + k, count - k),
             * k < count, is a leaf descriptor again — first + count <= 512 (nt <= 512 above says so already; held here in its own words) */
            if (n.left_or_first + n.triangle_count > 512u) return false;
            out = LDS_DESC_LEAF | (n.triangle_count << 9) | n.left_or_first;
            return true;
        }
        uint32_t l = n.left_or_first;
        if ((l & 1u) == 0u || (size_t)l + 1 >= nn) return false;
        out = (l >> 1) << 2;      /* the pair index times four: what the walk adds to its bases (k_walk.h lds_at) */
        return true;
    };
    if (!desc(nodes[0], root)) return false;
    for (size_t i = 0; i < nn; ++i)
        for (int k = 0; k < 3; ++k)
            if (!(nodes[i].aabb_min[k] <= nodes[i].aabb_max[k])) return false;
    const size_t P = (nn - 1) / 2, desc_vecs = (P + 3) / 4;
    pairs = (uint32_t)P;
    image.assign(6 * P + desc_vecs + 3 * nt, make_float4(0, 0, 0, 0));
    uint32_t *descs = reinterpret_cast<uint32_t *>(image.data() + 6 * P);
    for (size_t p = 0; p < P; ++p) {
        const rpt_bvh_node &L = nodes[2 * p + 1], &R = nodes[2 * p + 2];
        uint32_t dl, dr;
        if (!desc(L, dl) || !desc(R, dr)) return false;
        descs[p] = dl | (dr << 16);
        for (int k = 0; k < 3; ++k) {
            image[(2 * k) * P + p] = make_float4(L.aabb_min[k], R.aabb_min[k], L.aabb_max[k], R.aabb_max[k]);
            image[(2 * k + 1) * P + p] = make_float4(L.aabb_max[k], R.aabb_max[k], L.aabb_min[k], R.aabb_min[k]);
        }
    }
    for (size_t k = 0; k < 3 * nt; ++k) image[6 * P + desc_vecs + k] = geom[k];
    return true;
}

}  // namespace

/* The 64-byte pair records + per-node links of the streamed global-memory walks (k_walk.h SceneViewPairsT) from the uploaded node pool; with `flip`
 * (shadow_order.h) the two nodes of a flipped pair exchange slots: the copy the fixed-order shadow walks read.  (On the host this loop took 27 ms for 2 M nodes.) */
__global__ __launch_bounds__(RPT_BLOCK) void k_build_pairs(const float4 *nodes, const uint8_t *flip, uint32_t n_pairs, float4 *pairs, uint32_t *links) {
    const uint32_t p = blockIdx.x * RPT_BLOCK + threadIdx.x;
    auto link_of = [](float4 lo, float4 hi) { return (__float_as_uint(lo.w) << 24) | __float_as_uint(hi.w); };      /* triangle_count << 24 | left child / first triangle */
    if (p == 0u) links[0] = link_of(nodes[0], nodes[1]);
    if (p >= n_pairs) return;
    const bool f = flip != nullptr && flip[p] != 0;
    const uint32_t l = f ? 2u * p + 2u : 2u * p + 1u, r = f ? 2u * p + 1u : 2u * p + 2u;
    const float4 llo = nodes[2u * (size_t)l], lhi = nodes[2u * (size_t)l + 1u], rlo = nodes[2u * (size_t)r], rhi = nodes[2u * (size_t)r + 1u];
    const uint32_t kl = link_of(llo, lhi), kr = link_of(rlo, rhi);
    pairs[4u * (size_t)p + 0u] = make_float4(llo.x, llo.y, llo.z, lhi.x);
    pairs[4u * (size_t)p + 1u] = make_float4(lhi.y, lhi.z, rlo.x, rlo.y);
    pairs[4u * (size_t)p + 2u] = make_float4(rlo.z, rhi.x, rhi.y, rhi.z);
    pairs[4u * (size_t)p + 3u] = make_float4(0.0f, 0.0f, __uint_as_float(kl), __uint_as_float(kr));
    links[2u * p + 1u] = kl;
    links[2u * p + 2u] = kr;
}

/* tri_geom / tri_isect / tri_shade of every triangle (DevScene, k_common.h) and |e1 x e2|^2 for the shadow-order probe, from the uploaded reference buffers:
 *   tri_geom : a, e1 = b - a, e2 = c - a (muller_trumbore, intersection.rs:13-14; barycentric v0, v1, util.rs:239-240)
 *              with d00 = e1.e1, d01 = e1.e2, d11 = e2.e2 (util.rs:242-244) in the .w lanes — dot = (x x' + y y') + z z', as glam's
 *   tri_isect: e1, e2, a packed in 36 bytes        tri_shade: the three vertex normals, the three uv0 pairs and the material index in 64 bytes */
__global__ __launch_bounds__(RPT_BLOCK) void k_derive_triangles(const float4 *per_vertex, const uint4 *indices, uint32_t nt, float4 *tri_geom, float *tri_isect,
                                                                float4 *tri_shade, float4 *tri_tangent /* nullable */, float *cross_sq) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= nt) return;
    const uint4 t = indices[i];
    const float4 *A = per_vertex + 4u * (size_t)t.x, *B = per_vertex + 4u * (size_t)t.y, *C = per_vertex + 4u * (size_t)t.z;
    const float4 a = A[0], b = B[0], cc = C[0];
    const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
    const float e2x = cc.x - a.x, e2y = cc.y - a.y, e2z = cc.z - a.z;
    tri_geom[3u * (size_t)i + 0u] = make_float4(a.x, a.y, a.z, (e1x * e1x + e1y * e1y) + e1z * e1z);
    tri_geom[3u * (size_t)i + 1u] = make_float4(e1x, e1y, e1z, (e1x * e2x + e1y * e2y) + e1z * e2z);
    tri_geom[3u * (size_t)i + 2u] = make_float4(e2x, e2y, e2z, (e2x * e2x + e2y * e2y) + e2z * e2z);
    float *p = tri_isect + 9u * (size_t)i;
    p[0] = e1x; p[1] = e1y; p[2] = e1z; p[3] = e2x; p[4] = e2y; p[5] = e2z; p[6] = a.x; p[7] = a.y; p[8] = a.z;
    const float4 na = A[1], nb = B[1], nc = C[1], ua = A[3], ub = B[3], uc = C[3];
    tri_shade[4u * (size_t)i + 0u] = make_float4(na.x, na.y, na.z, ua.x);
    tri_shade[4u * (size_t)i + 1u] = make_float4(nb.x, nb.y, nb.z, ua.y);
    tri_shade[4u * (size_t)i + 2u] = make_float4(nc.x, nc.y, nc.z, __uint_as_float(t.w));
    tri_shade[4u * (size_t)i + 3u] = make_float4(ub.x, ub.y, uc.x, uc.y);
    if (tri_tangent) { tri_tangent[3u * (size_t)i + 0u] = A[2]; tri_tangent[3u * (size_t)i + 1u] = B[2]; tri_tangent[3u * (size_t)i + 2u] = C[2]; }
    const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;       /* (the probe's estimate of areas: no part of a result) */
    cross_sq[i] = (cx * cx + cy * cy) + cz * cz;
}

/* ---- the node pool as a tree, checked on the device (rpt_upload_scene) ------------------------------------------------------------------------------------------- */
struct NodeFacts {
    uint32_t error;        /* 1 child index out of bounds, 2 leaf range out of bounds, 4 a node reached twice, 8 deeper than 31 levels */
    uint32_t max_depth;
    uint32_t flags;        /* over ALL nodes of the pool: 1 a leaf of more than RPT_COOP_LEAF_MIN triangles, 2 a node the pair records cannot express, 4 a bound outside the exact-division guard */
};
constexpr uint32_t DEPTH_UNSET = 0xffffffffu;
/* pass p: the nodes at depth p claim their children for depth p + 1 (a child somebody already claimed: not a tree) */
__global__ __launch_bounds__(RPT_BLOCK) void k_validate_pass(const rpt_bvh_node *nodes, uint32_t nn, uint32_t nt, uint32_t *depth_of, uint32_t pass, NodeFacts *facts) {
    const uint32_t n = blockIdx.x * RPT_BLOCK + threadIdx.x;
    uint32_t err = 0u;
    const bool mine = n < nn && depth_of[n] == pass;
    if (mine) {
        const rpt_bvh_node node = nodes[n];
        if (pass > 31u) err = 8u;                  /* reference: FixedVec<usize, 32> would overflow (intersection.rs:178) */
        else if (node.triangle_count != 0u) { if ((size_t)node.left_or_first + node.triangle_count > nt) err = 2u; }
        else if ((size_t)node.left_or_first + 1 >= nn) err = 1u;
        else {
            if (atomicCAS(&depth_of[node.left_or_first], DEPTH_UNSET, pass + 1u) != DEPTH_UNSET) err = 4u;
            if (atomicCAS(&depth_of[node.left_or_first + 1u], DEPTH_UNSET, pass + 1u) != DEPTH_UNSET) err = 4u;
        }
    }
    const unsigned long long any = rpt_ballot(mine);
    if (any != 0ull && __lane_id() == (uint32_t)__ffsll((long long)any) - 1u && pass < 32u) facts->max_depth = pass;      /* (every writer of a launch stores the same value) */
    if (err != 0u) atomicOr(&facts->error, err);
}
__global__ __launch_bounds__(RPT_BLOCK) void k_node_flags(const rpt_bvh_node *nodes, uint32_t nn, NodeFacts *facts) {
    const uint32_t n = blockIdx.x * RPT_BLOCK + threadIdx.x;
    uint32_t bits = 0u;
    if (n < nn) {
        const rpt_bvh_node node = nodes[n];
        if (node.triangle_count > (uint32_t)RPT_COOP_LEAF_MIN) bits |= 1u;
        /* (an inner node's link names BOTH children: the right one, left_or_first + 1, has to fit the 24 bits too) */
        const uint32_t link_end = node.triangle_count == 0u ? (1u << 24) - 1u : (1u << 24);
        if (node.triangle_count >= 255u || node.left_or_first >= link_end || (node.triangle_count == 0u && ((node.left_or_first & 1u) == 0u || (size_t)node.left_or_first + 1 >= nn))) bits |= 2u;
        for (int k = 0; k < 3; ++k)
            if (!rptm::fastdiv_operand_ok(node.aabb_min[k]) || !rptm::fastdiv_operand_ok(node.aabb_max[k])) bits |= 4u;
    }
    uint32_t wave_bits = 0u;
    for (uint32_t b = 1u; b <= 4u; b <<= 1) if (rpt_ballot((bits & b) != 0u) != 0ull) wave_bits |= b;
    if (wave_bits != 0u && __lane_id() == 0u) atomicOr(&facts->flags, wave_bits);
}
/* nodes already on the device (not yet the context's); on RPT_OK `out` holds depth and flags */
static int device_validate_tree(rpt_ctx *c, const rpt_bvh_node *d_nodes, size_t nn, size_t nt, NodeFacts &out) {
    DevBuf<uint32_t> depth_of;
    DevBuf<NodeFacts> facts;
    HIP_TRY(c, depth_of.alloc(nn));
    HIP_TRY(c, facts.alloc(1));
    HIP_TRY(c, hipMemsetAsync(depth_of.p, 0xff, nn * sizeof(uint32_t), nullptr));
    HIP_TRY(c, hipMemsetAsync(depth_of.p, 0, sizeof(uint32_t), nullptr));              /* the root: depth 0 */
    HIP_TRY(c, hipMemsetAsync(facts.p, 0, sizeof(NodeFacts), nullptr));
    const unsigned blocks = rpt_blocks(nn);
    for (uint32_t pass = 0; pass <= 32u; ++pass) k_validate_pass<<<blocks, RPT_BLOCK>>>(d_nodes, (uint32_t)nn, (uint32_t)nt, depth_of.p, pass, facts.p);
    k_node_flags<<<blocks, RPT_BLOCK>>>(d_nodes, (uint32_t)nn, facts.p);
    HIP_TRY(c, hipMemcpy(&out, facts.p, sizeof(out), hipMemcpyDeviceToHost));
    HIP_TRY(c, hipGetLastError());
    if (out.error & 1u) { c->error = "BVH child index out of bounds"; return RPT_ESCENE; }
    if (out.error & 2u) { c->error = "BVH leaf range out of bounds"; return RPT_ESCENE; }
    if (out.error & 4u) { c->error = "BVH is not a tree"; return RPT_ESCENE; }
    if (out.error & 8u) { c->error = "BVH deeper than the reference's 32-entry traversal stack"; return RPT_ESCENE; }
    return RPT_OK;
}

/* what the pair records of the streamed global-memory walks (k_walk.h SceneViewPairsT) and the flipped copies can express: children of every inner node
 * are the nodes (2p + 1, 2p + 2) of one pair — every pool the reference's builder makes (src/bvh.rs:296-320) —, leaves of fewer than 255 triangles, and every index a
 * link stands for below 2^24: a leaf's first triangle, and BOTH children of an inner node (left_or_first + 1 < 2^24 — the walks push the right child's index, and a
 * 24-entry stack keeps 24 bits of it: node 2^24 would come back as node 0, the root).
 * `every_node_fits`: no node of the pool has bit 2 of NodeFacts::flags (k_node_flags on the device, the loop below on the host) */
static bool pool_is_pair_shaped(const rpt_bvh_node *nodes, size_t nn, bool every_node_fits) {
    return (nn & 1u) == 1u && nn >= 3 && nodes[0].triangle_count == 0u && every_node_fits;
}
/* (the host debug hooks, which have no device: bit 2 of k_node_flags, node by node) */
static bool pool_is_pair_shaped(const rpt_bvh_node *nodes, size_t nn) {
    bool fits = true;
    for (size_t i = 0; i < nn && fits; ++i) {
        const rpt_bvh_node &n = nodes[i];
        const uint32_t link_end = n.triangle_count == 0u ? (1u << 24) - 1u : (1u << 24);
        fits = n.triangle_count < 255u && n.left_or_first < link_end && (n.triangle_count != 0u || ((n.left_or_first & 1u) != 0u && (size_t)n.left_or_first + 1 < nn));
    }
    return pool_is_pair_shaped(nodes, nn, fits);
}

/* One rpt_upload_scene call: the caller's buffers and what its steps learn for the steps after them.  The steps read sizes from here, never from
 * c->scene: its flags are written by the step that decides each of them, its pointers and counts by bind_scene, once, when every buffer is in place. */
struct Upload {
    const rpt_per_vertex_data *pv; size_t nv; const rpt_triangle *idx; size_t nt; const rpt_bvh_node *nodes; size_t nn;
    const rpt_material_data *mats; size_t nm; const rpt_light_pick_entry *lp; size_t nlp;
    const uint8_t *atlas; uint32_t aw, ah; const float *skybox; uint32_t sw, sh;
    SectionTimer sections{"rpt_upload_scene"};
    DevBuf<float4> new_nodes;          /* the pool on the device, not yet the context's */
    NodeFacts facts{};
    std::vector<float4> geom;          /* tri_geom on the host: only for a scene small enough for the LDS image, whose builder reads it */
    bool lds_candidate = false, pair_shaped = false, want_last = false;
    uint32_t n_pairs = 0;
    DevBuf<float> cross_sq;            /* |e1 x e2|^2 per triangle: the order probes' triangle areas (freed as soon as they ran) */
    bool lights() const { return !(lp[0].ratio < 0.0f); }
};

/* ---- the order probes as kernels (shadow_order.h: the core is shared with the host driver) ---------------------------------------------------------------- */
namespace order_probe {

constexpr uint32_t LEVEL_UNSET = 0xffffffffu;
struct DevStack {
    uint32_t *column;                                   /* LDS [entry][lane] */
    __device__ __forceinline__ uint32_t &operator()(int k) const { return column[k * RPT_WAVE]; }
};

__global__ __launch_bounds__(RPT_BLOCK) void k_probe_tri_area(const float *cross_sq, uint32_t nt, double *tri_area) {
    const uint32_t t = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (t < nt) tri_area[t] = area_of_cross_sq(cross_sq[t]);
}
/* leaves: the sums over their own triangles, in index order (as host_sums adds them); inner nodes wait for their children */
__global__ __launch_bounds__(RPT_BLOCK) void k_probe_leaves(View s, double *area_all, double *area_ne, double *count, uint32_t *level) {
    const uint32_t n = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (n >= s.nn) return;
    const rpt_bvh_node &node = s.nodes[n];
    count[n] = 1.0;
    if (node.triangle_count == 0u) { level[n] = LEVEL_UNSET; return; }
    double a = 0.0, ne = 0.0;
    for (uint32_t k = 0; k < node.triangle_count; ++k) {
        const uint32_t t = node.left_or_first + k;
        a += s.tri_area[t];
        if (!emissive(s, t)) ne += s.tri_area[t];
    }
    area_all[n] = a; area_ne[n] = ne; level[n] = 0u;
}
/* pass p: the inner nodes whose children were both finished by EARLIER launches (level < p: nothing read here is written by this launch) */
__global__ __launch_bounds__(RPT_BLOCK) void k_probe_inner(View s, double *area_all, double *area_ne, double *count, uint32_t *level, uint32_t pass) {
    const uint32_t n = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (n >= s.nn || level[n] != LEVEL_UNSET) return;
    const uint32_t L = s.nodes[n].left_or_first, R = L + 1u;
    if (level[L] >= pass || level[R] >= pass) return;
    area_all[n] = area_all[L] + area_all[R];
    area_ne[n] = area_ne[L] + area_ne[R];
    count[n] = 1.0 + count[L] + count[R];
    level[n] = pass;
}
__global__ __launch_bounds__(RPT_BLOCK) void k_probe_flips(View s, uint32_t n_pairs, uint8_t *flip1, uint8_t *flip2, uint8_t *flip3) {
    const uint32_t p = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (p >= n_pairs) return;
    flip1[p] = prefers_right(s, p, 1) ? 1 : 0;
    if (flip2) { flip2[p] = prefers_right(s, p, 2) ? 1 : 0; flip3[p] = prefers_right(s, p, 3) ? 1 : 0; }
}
/* PROBE_LANES adjacent lanes per (probe ray, order): they take every decision together (the same registers, redundantly) and split the triangles of a leaf — one thread per
 * walk spent 5.8 ms on the clustered stand-in's 64-triangle leaves, whatever the GPU's width.  Job 2i walks ray i near child first, job 2i + 1 in the fixed order;
 * counters: node visits near first, fixed, rays, occluded */
constexpr uint32_t PROBE_LANES = 8u;
__global__ __launch_bounds__(RPT_WAVE) void k_probe_shadow(View s, const uint8_t *flip, unsigned long long *counters) {
    __shared__ uint32_t stacks[ORDER_PROBE_STACK * RPT_WAVE];
    const uint32_t job = (blockIdx.x * RPT_WAVE + threadIdx.x) / PROBE_LANES, i = job >> 1;
    s.sub = threadIdx.x % PROBE_LANES;
    s.lanes = PROBE_LANES;
    const bool all = !(s.area_ne[0] > 0.0);
    if (i >= SHADOW_PROBE_RAYS || (all && !(s.area_all[0] > 0.0))) return;
    V o, d;
    float max_t;
    if (!shadow_probe_ray(s, all, i, o, d, max_t)) return;
    bool occluded = false;
    const DevStack stack{stacks + threadIdx.x};
    const uint32_t visits = (job & 1u) == 0u ? walk<false>(s, flip, o, d, max_t, stack, occluded) : walk<true>(s, flip, o, d, max_t, stack, occluded);
    if (s.sub != 0u) return;
    if ((job & 1u) == 0u) {
        atomicAdd(&counters[0], (unsigned long long)visits);
        atomicAdd(&counters[2], 1ull);
        if (occluded) atomicAdd(&counters[3], 1ull);
    } else {
        atomicAdd(&counters[1], (unsigned long long)visits);
    }
}
/* PROBE_LANES lanes per (probe ray, order 0..3); counters 4..7: node visits near first and under rules 1..3; 8: rays; 9: hits */
__global__ __launch_bounds__(RPT_WAVE) void k_probe_last(View s, const uint8_t *flip1, const uint8_t *flip2, const uint8_t *flip3, unsigned long long *counters) {
    __shared__ uint32_t stacks[ORDER_PROBE_STACK * RPT_WAVE];
    const uint32_t job = (blockIdx.x * RPT_WAVE + threadIdx.x) / PROBE_LANES, i = job >> 2, q = job & 3u;
    s.sub = threadIdx.x % PROBE_LANES;
    s.lanes = PROBE_LANES;
    if (i >= LAST_PROBE_RAYS || !(s.area_ne[0] > 0.0)) return;
    V o, d;
    if (!last_probe_ray(s, i, o, d)) return;
    bool hit = false;
    const DevStack stack{stacks + threadIdx.x};
    const uint8_t *flip = q == 1u ? flip1 : (q == 2u ? flip2 : flip3);
    const uint32_t visits = q == 0u ? walk<false>(s, nullptr, o, d, 1000000.0f, stack, hit) : walk<true>(s, flip, o, d, 1000000.0f, stack, hit);
    if (s.sub != 0u) return;
    atomicAdd(&counters[4u + q], (unsigned long long)visits);
    if (q == 3u) {                                        /* (the host loop reports the hit flag of its last walk: rule 3) */
        atomicAdd(&counters[8], 1ull);
        if (hit) atomicAdd(&counters[9], 1ull);
    }
}

}  // namespace order_probe

/* Both decisions of shadow_order.h for the scene just uploaded into `c`, on the device: the same rays, the same node visits and therefore the same decision
 * as choose_shadow_order / choose_last_order make on the host (tests/test_gpu_parity.py compares them to the last digit).  u.cross_sq: what k_derive_triangles
 * left.  Kernels on the null stream, like the other upload-time kernels. */
static int device_order_probes(rpt_ctx *c, const Upload &u, ShadowOrder &so, LastOrder &lo) {
    using namespace order_probe;
    const Clock clock;
    so = ShadowOrder();
    lo = LastOrder();
    const uint32_t nt = (uint32_t)u.nt, nn = (uint32_t)u.nn, P = nn >= 3u ? (nn - 1u) / 2u : 0u, depth = u.facts.max_depth;
    const bool lights = u.lights(), want_last = u.want_last;
    if (nt == 0u || (!lights && !want_last)) { so.probe_ms = lo.probe_ms = clock.ms(); return RPT_OK; }
    if (!u.pair_shaped || nn < 3u) { if (lights) so.why = "node pool is not pair-shaped"; so.probe_ms = lo.probe_ms = clock.ms(); return RPT_OK; }
    constexpr const char *WHERE = "order probes: ";               /* prefix of the HIP error messages */
    /* ONE allocation, carved up (five hipMalloc / hipFree pairs were a third of the probe's 5 ms on a 1 M-triangle scene) */
    Arena arena;
    const size_t bytes = Arena::pad((size_t)nt * sizeof(double)) + Arena::pad(3 * (size_t)nn * sizeof(double)) + Arena::pad((size_t)nn * sizeof(uint32_t)) +
                         Arena::pad(3 * (size_t)P) + Arena::pad(10 * sizeof(unsigned long long));
    HIP_TRY_TO(c->error, WHERE, arena.reserve(bytes));
    double *tri_area = arena.take<double>(nt), *sums = arena.take<double>(3 * (size_t)nn);
    uint32_t *level = arena.take<uint32_t>(nn);
    uint8_t *flips = arena.take<uint8_t>(3 * (size_t)P);
    unsigned long long *counters = arena.take<unsigned long long>(10);
    HIP_TRY_TO(c->error, WHERE, hipMemsetAsync(counters, 0, 10 * sizeof(unsigned long long), nullptr));
    double *area_all = sums, *area_ne = sums + nn, *count = sums + 2 * (size_t)nn;
    const View s{reinterpret_cast<const rpt_per_vertex_data *>(c->per_vertex.p), reinterpret_cast<const rpt_triangle *>(c->indices.p),
                 reinterpret_cast<const rpt_bvh_node *>(c->nodes.p), reinterpret_cast<const rpt_material_data *>(c->materials.p), c->light_pick.p, nt, nn,
                 (uint32_t)u.nlp, tri_area, area_all, area_ne, count, 0u, 1u, reinterpret_cast<const float4_like *>(c->tri_geom.p)};
    const unsigned node_blocks = rpt_blocks(nn);
    k_probe_tri_area<<<rpt_blocks(nt), RPT_BLOCK>>>(u.cross_sq.p, nt, tri_area);
    k_probe_leaves<<<node_blocks, RPT_BLOCK>>>(s, area_all, area_ne, count, level);
    for (uint32_t pass = 1; pass <= depth; ++pass) k_probe_inner<<<node_blocks, RPT_BLOCK>>>(s, area_all, area_ne, count, level, pass);
    uint8_t *flip1 = flips, *flip2 = want_last ? flips + P : nullptr, *flip3 = want_last ? flips + 2 * (size_t)P : nullptr;
    k_probe_flips<<<rpt_blocks(P), RPT_BLOCK>>>(s, P, flip1, flip2, flip3);
    if (lights) k_probe_shadow<<<2 * SHADOW_PROBE_RAYS * PROBE_LANES / RPT_WAVE, RPT_WAVE>>>(s, flip1, counters);
    if (want_last) k_probe_last<<<4 * LAST_PROBE_RAYS * PROBE_LANES / RPT_WAVE, RPT_WAVE>>>(s, flip1, flip2, flip3, counters);
    unsigned long long h[10];
    HIP_TRY_TO(c->error, WHERE, hipMemcpy(h, counters, sizeof(h), hipMemcpyDeviceToHost));       /* (waits for the kernels) */
    HIP_TRY_TO(c->error, WHERE, hipGetLastError());
    if (lights) {
        decide_shadow(so, h[0], h[1], (uint32_t)h[2], (uint32_t)h[3], c->knobs.shadow_order);
        so.flip.assign(P, 0);
        if (so.fixed) HIP_TRY_TO(c->error, WHERE, hipMemcpy(so.flip.data(), flip1, P, hipMemcpyDeviceToHost));
    }
    if (want_last) {
        const uint64_t v[4] = {h[4], h[5], h[6], h[7]};
        decide_last(lo, v, (uint32_t)h[8], (uint32_t)h[9], c->knobs.last_order);
        if (lo.rule != 0) {
            lo.flip.assign(P, 0);
            HIP_TRY_TO(c->error, WHERE, hipMemcpy(lo.flip.data(), flips + (size_t)(lo.rule - 1) * P, P, hipMemcpyDeviceToHost));
        }
    }
    arena.mem.release();                 /* (inside the probe time, which has always counted the free) */
    so.probe_ms = lo.probe_ms = clock.ms();
    return RPT_OK;
}

/* The LDS traversal image of the context's node pool (`flip` null) or of its copy with the pairs `flip` marks flipped, into `dst`.  The primary image goes
 * up if it fits RPT_LDS_SCENE_BYTES and sets the scene's lds_pairs / lds_vecs / lds_root; a flipped copy only if it has that same size, pairs and root (the
 * walks address both alike), and only its first `keep` vectors.  `built`: whether `dst` now holds it (otherwise nothing was allocated). */
static int upload_lds_image(rpt_ctx *c, const Upload &u, const std::vector<uint8_t> *flip, size_t keep, DevBuf<float4> &dst, bool &built) {
    DevScene &s = c->scene;
    const std::vector<rpt_bvh_node> pool = flip ? flipped_nodes(u.nodes, u.nn, *flip) : std::vector<rpt_bvh_node>();
    std::vector<float4> image;
    uint32_t pairs = 0, root = 0;
    built = build_lds_image(flip ? pool.data() : u.nodes, u.nn, u.geom, u.nt, image, pairs, root) &&
            (flip ? image.size() == (size_t)s.lds_vecs && pairs == s.lds_pairs && root == s.lds_root : image.size() * sizeof(float4) <= RPT_LDS_SCENE_BYTES);
    if (!built) return RPT_OK;
    const size_t n = std::min(keep, image.size());
    HIP_TRY(c, dst.alloc(std::max<size_t>(1, n)));
    if (n) HIP_TRY(c, hipMemcpy(dst.p, image.data(), n * sizeof(float4), hipMemcpyHostToDevice));
    if (!flip) { s.lds_pairs = pairs; s.lds_vecs = (uint32_t)image.size(); s.lds_root = root; }
    return RPT_OK;
}

/* pair records + links of the streamed global-memory walks (k_walk.h SceneViewPairsT) over the context's node pool, with the pairs `flip` marks
 * flipped (null: none) */
static int build_pair_records(rpt_ctx *c, const Upload &u, const std::vector<uint8_t> *flip, DevBuf<float4> &pairs, DevBuf<uint32_t> &links) {
    const uint32_t n_pairs = u.n_pairs;
    DevBuf<uint8_t> d_flip;
    if (flip) {
        HIP_TRY(c, d_flip.alloc(std::max<size_t>(1, flip->size())));
        HIP_TRY(c, hipMemcpy(d_flip.p, flip->data(), flip->size(), hipMemcpyHostToDevice));
    }
    HIP_TRY(c, pairs.alloc(std::max<size_t>(1, 4 * (size_t)n_pairs)));
    HIP_TRY(c, links.alloc(u.nn));
    k_build_pairs<<<rpt_blocks(n_pairs), RPT_BLOCK>>>(c->nodes.p, d_flip.p, n_pairs, pairs.p, links.p);
    if (flip) HIP_TRY(c, hipDeviceSynchronize());          /* (before d_flip is freed) */
    else HIP_TRY(c, hipGetLastError());
    return RPT_OK;
}

/* ---- rpt_upload_scene, step by step: each returns an RPT_* code, the driver at the end runs them in the order they stand here ------------------------------------ */

/* what is refused before anything is touched: sizes and indices, a missing or oversized atlas */
static int check_arguments(rpt_ctx *c, Upload &u) {
    RPT_TRY(validate_scene_flat(c, u.pv, u.nv, u.idx, u.nt, u.nn, u.mats, u.nm, u.lp, u.nlp));
    for (size_t i = 0; i < u.nm; ++i)
        if ((u.mats[i].has_albedo_texture | u.mats[i].has_metallic_texture | u.mats[i].has_roughness_texture | u.mats[i].has_normal_texture) &&
            (!u.atlas || !u.aw || !u.ah)) {
            c->error = "a material references the texture atlas but no atlas was supplied";
            return RPT_ESCENE;
        }
    /* texel indices are 32-bit on the device (k_shade.h sample_by_lod): the reference's atlas is 4096 x 4096 (src/asset.rs:177) */
    if ((u.atlas && (uint64_t)u.aw * u.ah > (1ull << 30)) || (u.skybox && (uint64_t)u.sw * u.sh > (1ull << 28))) {
        c->error = "atlas larger than 2^30 texels / skybox larger than 2^28 texels";
        return RPT_ESCENE;
    }
    u.sections.mark("validate_flat");
    return RPT_OK;
}

/* the node pool goes up first, into a buffer of its own: it is checked on the device (a tree, in range, at most 31 levels: device_validate_tree) before the
 * context's scene is touched — a rejected upload leaves the previous scene in place */
static int stage_nodes(rpt_ctx *c, Upload &u) {
    HIP_TRY(c, u.new_nodes.from_host(u.nodes, 2 * u.nn));
    RPT_TRY(device_validate_tree(c, reinterpret_cast<const rpt_bvh_node *>(u.new_nodes.p), u.nn, u.nt, u.facts));
    u.lds_candidate = u.nn * 50 + u.nt * 48 <= RPT_LDS_SCENE_BYTES && u.facts.max_depth <= 15;
    /* a pool the pair records cannot express keeps the one-shot walks */
    u.pair_shaped = pool_is_pair_shaped(u.nodes, u.nn, (u.facts.flags & 2u) == 0u);
    u.n_pairs = u.pair_shaped ? (uint32_t)((u.nn - 1) / 2) : 0u;
    u.sections.mark("validate_tree_device");
    return RPT_OK;
}

/* From here until the driver's last line the context has no scene.  The optional structures of the previous one are released now: the steps below allocate
 * what THIS scene gets, and a buffer nobody allocated has p == nullptr — exactly what bind_scene has to hand the kernels for "not there". */
static int begin_scene(rpt_ctx *c, Upload &u) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->has_scene = false;
    c->lds_image.release(); c->lds_image_shadow.release(); c->lds_image_last.release();
    c->gpairs.release(); c->glinks.release(); c->gpairs_shadow.release(); c->glinks_shadow.release();
    c->fat_leaves = (u.facts.flags & 1u) != 0u;
    if (c->knobs.coop_leaves >= 0) c->fat_leaves = c->knobs.coop_leaves != 0;
    c->scene.fastdiv_ok = (u.facts.flags & 4u) == 0u ? 1u : 0u;          /* every node bound is 0 or in [2^-60, 2^40) (k_node_flags) */
    return RPT_OK;
}

/* Vertices, indices, materials and light-pick entries as they came, mat_lite (emissive / albedo colours + roughness.x / metallic.x in 32 bytes, for
 * untextured scenes) and the derived per-triangle records, computed with the very f32 operations the reference performs per hit — ON THE DEVICE
 * (k_derive_triangles, which describes them: the host loops over a million triangles, three scattered 64-byte vertices each, and the transfer of their
 * 148 bytes per triangle were 90 ms of a 1 M-triangle upload, profiles/r05_startup_sections.txt).  The host derives `geom` itself only for a scene
 * small enough for the LDS image, whose builder reads it. */
static int upload_geometry(rpt_ctx *c, Upload &u) {
    const size_t nt = u.nt, nm = u.nm;
    std::vector<float4> lite(2 * nm);
    if (u.lds_candidate) {
        auto dot = [](const float *a, const float *b) { return (a[0] * b[0]) + (a[1] * b[1]) + (a[2] * b[2]); };
        u.geom.resize(3 * nt);
        for (size_t i = 0; i < nt; ++i) {
            const float *a = u.pv[u.idx[i].v0].vertex, *b = u.pv[u.idx[i].v1].vertex, *cc = u.pv[u.idx[i].v2].vertex;
            float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
            float e2[3] = {cc[0] - a[0], cc[1] - a[1], cc[2] - a[2]};
            u.geom[3 * i + 0] = make_float4(a[0], a[1], a[2], dot(e1, e1));
            u.geom[3 * i + 1] = make_float4(e1[0], e1[1], e1[2], dot(e1, e2));
            u.geom[3 * i + 2] = make_float4(e2[0], e2[1], e2[2], dot(e2, e2));
        }
    }
    bool normal_maps = false;
    c->scene.textured = 0u;
    for (size_t i = 0; i < nm; ++i) {
        const rpt_material_data &m = u.mats[i];
        if (m.has_normal_texture) normal_maps = true;
        lite[2 * i + 0] = make_float4(m.emissive[0], m.emissive[1], m.emissive[2], m.roughness[0]);
        lite[2 * i + 1] = make_float4(m.albedo[0], m.albedo[1], m.albedo[2], m.metallic[0]);
        if (m.has_albedo_texture | m.has_metallic_texture | m.has_roughness_texture | m.has_normal_texture) c->scene.textured = 1u;
    }
    u.sections.mark("derive_host");
    c->nodes = std::move(u.new_nodes);
    HIP_TRY(c, c->tri_geom.alloc(3 * nt));
    HIP_TRY(c, c->tri_shade.alloc(4 * nt));
    HIP_TRY(c, c->tri_isect.alloc(9 * nt));
    HIP_TRY(c, c->tri_tangent.alloc(normal_maps ? 3 * nt : 0));
    HIP_TRY(c, u.cross_sq.alloc(nt));
    HIP_TRY(c, c->per_vertex.from_host(u.pv, 4 * u.nv));
    HIP_TRY(c, c->indices.from_host(u.idx, nt));
    if (nt) k_derive_triangles<<<rpt_blocks(nt), RPT_BLOCK>>>(c->per_vertex.p, c->indices.p, (uint32_t)nt, c->tri_geom.p, c->tri_isect.p, c->tri_shade.p, c->tri_tangent.p, u.cross_sq.p);
    HIP_TRY(c, c->mat_lite.from_host(lite.data(), lite.size()));
    HIP_TRY(c, c->materials.from_host(u.mats, 6 * nm));
    HIP_TRY(c, c->light_pick.from_host(u.lp, u.nlp));
    HIP_TRY(c, hipGetLastError());
    u.sections.mark("h2d_derive_device");
    return RPT_OK;
}

/* per light-pick entry, for its two triangles: corners, the mean of the three vertex normals exactly as
 * sample_direct_lighting forms it ((na + nb + nc) / 3.0, light_pick.rs:129), and the material's emission */
static int upload_light_records(rpt_ctx *c, Upload &u) {
    std::vector<float4> rec(8 * u.nlp, make_float4(0, 0, 0, 0));
    if (u.lights())
        for (size_t i = 0; i < u.nlp; ++i)
            for (int side = 0; side < 2; ++side) {
                const uint32_t t = side ? u.lp[i].triangle_index_b : u.lp[i].triangle_index_a;
                const rpt_per_vertex_data &A = u.pv[u.idx[t].v0], &B = u.pv[u.idx[t].v1], &C = u.pv[u.idx[t].v2];
                float n[3];
                for (int k = 0; k < 3; ++k) n[k] = ((A.normal[k] + B.normal[k]) + C.normal[k]) / 3.0f;
                const float *em = u.mats[u.idx[t].material].emissive;
                float4 *r = &rec[8 * i + 4 * side];
                r[0] = make_float4(A.vertex[0], A.vertex[1], A.vertex[2], n[0]);
                r[1] = make_float4(B.vertex[0], B.vertex[1], B.vertex[2], n[1]);
                r[2] = make_float4(C.vertex[0], C.vertex[1], C.vertex[2], n[2]);
                r[3] = make_float4(em[0], em[1], em[2], 0.0f);
            }
    HIP_TRY(c, c->light_rec.from_host(rec.data(), rec.size()));
    c->scene.no_lights = u.lights() ? 0u : 1u;
    u.sections.mark("h2d_2_light_rec");
    return RPT_OK;
}

/* atlas and skybox; where the caller has none, the reference's 2 x 2 magenta stand-in (`u` then names it) */
static int upload_images(rpt_ctx *c, Upload &u) {
    static const uint8_t magenta_u8[16] = {255, 0, 255, 255, 255, 0, 255, 255, 255, 0, 255, 255, 255, 0, 255, 255};
    static const float magenta_f[16] = {1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1};   /* src/asset.rs:283-290 */
    if (!u.atlas || !u.aw || !u.ah) { u.atlas = magenta_u8; u.aw = u.ah = 2; }
    if (!u.skybox || !u.sw || !u.sh) { u.skybox = magenta_f; u.sw = u.sh = 2; }
    HIP_TRY(c, c->atlas.from_host(u.atlas, (size_t)u.aw * u.ah));
    HIP_TRY(c, c->skybox.from_host(u.skybox, (size_t)u.sw * u.sh));
    return RPT_OK;
}

/* what the walks read instead of the node pool: the LDS image of a small scene, the pair records of the streamed global-memory walks (k_walk.h) */
static int build_walk_structures(rpt_ctx *c, Upload &u) {
    DevScene &s = c->scene;
    s.lds_scene = 0u; s.lds_pairs = s.lds_vecs = s.lds_root = 0u;
    if (u.lds_candidate) {
        bool built = false;
        RPT_TRY(upload_lds_image(c, u, nullptr, SIZE_MAX, c->lds_image, built));
        s.lds_scene = built ? 1u : 0u;
    }
    u.sections.mark("atlas_lds_image");
    if (c->knobs.no_lds_scene) s.lds_scene = 0u;          /* (the image stays where it is, and bound: only the walks ignore it) */
    if (u.pair_shaped) RPT_TRY(build_pair_records(c, u, nullptr, c->gpairs, c->glinks));
    u.sections.mark("pairs");
    return RPT_OK;
}

/* The last extension rays of a batch without NEE only have to say "hit or miss" unless they can end on an emitter (k_traverse_nearest.h
 * k_traverse_nearest_stream LAST): the triangles whose material emits (lib.rs:86: emissive.xyz() != 0, a NaN counts), if they are few enough to test
 * each ray against.  Then both order decisions by probe rays, as kernels over the buffers just uploaded (shadow_order.h; round 5 walked the rays on the
 * host: 17 - 40 ms of a 1 M-triangle upload). */
static int probe_orders(rpt_ctx *c, Upload &u) {
    DevScene &s = c->scene;
    s.last_emit_n = 0u;
    for (uint32_t k = 0; k < RPT_LAST_EMIT_MAX; ++k) s.last_emit_tri[k] = 0u;
    for (size_t t = 0; t < u.nt && s.last_emit_n <= RPT_LAST_EMIT_MAX; ++t) {
        const float *e = u.mats[u.idx[t].material].emissive;
        if (!(e[0] == 0.0f && e[1] == 0.0f && e[2] == 0.0f)) {
            if (s.last_emit_n < RPT_LAST_EMIT_MAX) s.last_emit_tri[s.last_emit_n] = (uint32_t)t;
            s.last_emit_n += 1u;
        }
    }
    if (c->knobs.last_order == 4) s.last_emit_n = RPT_LAST_EMIT_MAX + 1u;      /* RPT_LAST_ORDER=off (A/B and tests): the plain launch */
    u.want_last = s.lds_scene && s.last_emit_n <= RPT_LAST_EMIT_MAX;
    const int rc = device_order_probes(c, u, c->shadow_order, c->last_order);
    u.cross_sq.release();
    return rc;
}

/* The any-hit (shadow) walks may visit siblings in any order (shadow_order.h: only `.hit` is read, light_pick.rs:148).  Where the probe chose the fixed
 * opaque-first order over the reference's near-first one, they walk a copy of the tree whose pairs are flipped so that the preferred child is the LEFT
 * one: a second LDS image / pair array, read by the shadow kernels only. */
static int upload_shadow_copies(rpt_ctx *c, Upload &u) {
    DevScene &s = c->scene;
    s.shadow_fixed = 0u;
    if (c->shadow_order.fixed) {
        bool built = false;
        if (s.lds_scene) RPT_TRY(upload_lds_image(c, u, &c->shadow_order.flip, SIZE_MAX, c->lds_image_shadow, built));
        if (u.pair_shaped) {
            RPT_TRY(build_pair_records(c, u, &c->shadow_order.flip, c->gpairs_shadow, c->glinks_shadow));
            built = true;
        }
        s.shadow_fixed = built ? 1u : 0u;
    }
    u.sections.mark("shadow_order");
    return RPT_OK;
}

/* The order the last extension rays walk in (shadow_order.h): near child first over the primary image, or a fixed order over a copy whose pairs are
 * flipped by the rule that needed the fewest node visits on probe rays of their kind — if there is room behind the LDS image for that copy's pair records. */
static int upload_last_copy(rpt_ctx *c, Upload &u) {
    DevScene &s = c->scene;
    s.last_flip_vecs = 0u;
    if (u.want_last) {
        const size_t flip_vecs = 6 * (size_t)s.lds_pairs + ((size_t)s.lds_pairs + 3) / 4;
        /* room: two 1 024-thread workgroups per CU (k_walk_stream.h), i.e. half of what THIS device's CU holds (160 KB on MI355X; a partitioned or older device
         * reports less and simply gets no flipped copy), minus the kernel's static LDS as the code object states it */
        size_t lds_room = 0;
        hipDeviceProp_t prop;
        hipFuncAttributes fa;
        if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.maxSharedMemoryPerMultiProcessor != 0 && rpt_last_walk_attributes(&fa) == hipSuccess) {
            const size_t per_wg = prop.maxSharedMemoryPerMultiProcessor / 2;
            lds_room = per_wg > fa.sharedSizeBytes ? per_wg - fa.sharedSizeBytes : 0;
        }
        if (c->last_order.rule != 0 && ((size_t)s.lds_vecs + flip_vecs) * sizeof(float4) <= lds_room) {
            bool built = false;
            RPT_TRY(upload_lds_image(c, u, &c->last_order.flip, flip_vecs, c->lds_image_last, built));
            if (built) s.last_flip_vecs = (uint32_t)flip_vecs;
        }
        if (!c->lds_image_last.p) c->last_order.rule = 0;
    }
    u.sections.mark("last_order");
    return RPT_OK;
}

/* THE place where DevScene learns where the scene's buffers are and how large: every pointer and count, the optional structures as null where this
 * scene has none (begin_scene released them, no step allocated them) */
static void bind_scene(rpt_ctx *c, const Upload &u) {
    DevScene &s = c->scene;
    s.nodes = c->nodes.p; s.tri_geom = c->tri_geom.p; s.tri_isect = c->tri_isect.p; s.tri_shade = c->tri_shade.p; s.tri_tangent = c->tri_tangent.p; s.mat_lite = c->mat_lite.p;
    s.indices = c->indices.p; s.per_vertex = c->per_vertex.p;
    s.materials = c->materials.p; s.light_pick = c->light_pick.p; s.light_rec = c->light_rec.p;
    s.n_light_pick = (uint32_t)u.nlp; s.n_nodes = (uint32_t)u.nn; s.n_triangles = (uint32_t)u.nt;
    s.lds_image = c->lds_image.p; s.gpairs = c->gpairs.p; s.glinks = c->glinks.p;
    s.lds_image_shadow = c->lds_image_shadow.p; s.gpairs_shadow = c->gpairs_shadow.p; s.glinks_shadow = c->glinks_shadow.p;
    s.lds_image_last = c->lds_image_last.p;
    s.atlas = DevImage{c->atlas.p, u.aw, u.ah};
    s.skybox = DevImage{c->skybox.p, u.sw, u.sh};
}

extern "C" {

int rpt_upload_scene(rpt_ctx *c, const rpt_per_vertex_data *pv, size_t nv, const rpt_triangle *idx, size_t nt,
                     const rpt_bvh_node *nodes, size_t nn, const rpt_material_data *mats, size_t nm,
                     const rpt_light_pick_entry *lp, size_t nlp, const uint8_t *atlas, uint32_t aw, uint32_t ah,
                     const float *skybox, uint32_t sw, uint32_t sh) {
    if (!c) return RPT_EINVAL;
    if (!pv || !idx || !nodes || !mats || !lp) { c->error = "null scene buffer"; return RPT_EINVAL; }
    HIP_TRY(c, hipSetDevice(c->device));
    {   /* the knobs that act at upload (orders, leaf build, LDS residency) are read again: a test process changes them between scenes of one context */
        const rpt_knobs now = rpt_read_knobs();
        c->knobs.shadow_order = now.shadow_order; c->knobs.last_order = now.last_order; c->knobs.coop_leaves = now.coop_leaves; c->knobs.no_lds_scene = now.no_lds_scene;
    }
    Upload u{pv, nv, idx, nt, nodes, nn, mats, nm, lp, nlp, atlas, aw, ah, skybox, sw, sh};
    int (*const steps[])(rpt_ctx *, Upload &) = {check_arguments, stage_nodes /* up to here a refused upload leaves the previous scene in place */,
                                                 begin_scene, upload_geometry, upload_light_records, upload_images, build_walk_structures,
                                                 probe_orders, upload_shadow_copies, upload_last_copy};
    for (auto step : steps) RPT_TRY(step(c, u));
    bind_scene(c, u);
    u.sections.mark("fastdiv_check");
    HIP_TRY(c, hipStreamSynchronize(nullptr));                 /* the derive / pair kernels ran on the null stream; the context renders on its own */
    HIP_TRY(c, hipGetLastError());
    c->bvh_depth = u.facts.max_depth;
    /* the 16-entry stack has 16-bit entries and nothing wider (rpt_traverse.hip with_stack_width): it takes a tree of at most 15 levels in a pool of fewer than 65 536
     * nodes.  A sparse pool can be that shallow and still link to node 65 536 and beyond: it walks with 24 entries, whose widths follow the node count. */
    c->stack_cap = c->bvh_depth <= 15 && nn < 65536u ? 16 : (c->bvh_depth <= 23 ? 24 : 32);
    c->has_scene = true;
    c->n_materials = (uint32_t)nm;
    rpt_material_models_clear(c);        /* the records belong to the materials of the scene that was */
    rpt_material_volumes_clear(c);
    rpt_punctual_lights_clear(c);
    c->dn.guides_valid = false;          /* the denoiser's guides are first hits in THIS scene */
    c->dn.scene_changed = true;          /* ... and so is the history of rpt_denoise_temporal: its next call drops it */
    return RPT_OK;
}

int rpt_shadow_order(rpt_ctx *c, uint32_t *fixed_out, double *visits_near_out, double *visits_fixed_out, uint32_t *probe_rays_out, double *probe_ms_out) {
    if (!c) return RPT_EINVAL;
    if (!c->has_scene) { c->error = "rpt_shadow_order: no scene"; return RPT_EINVAL; }
    if (fixed_out) *fixed_out = c->scene.shadow_fixed;
    if (visits_near_out) *visits_near_out = c->shadow_order.visits_near;
    if (visits_fixed_out) *visits_fixed_out = c->shadow_order.visits_fixed;
    if (probe_rays_out) *probe_rays_out = c->shadow_order.probe_rays;
    if (probe_ms_out) *probe_ms_out = c->shadow_order.probe_ms;
    return RPT_OK;
}

/* the same decision without a device (tests: the probe is host code) */
int rpt_last_bounce_order(rpt_ctx *c, uint32_t *mode_out, uint32_t *n_emissive_out, double *visits_out, uint32_t *probe_rays_out, double *probe_ms_out) {
    if (!c) return RPT_EINVAL;
    if (!c->has_scene) { c->error = "rpt_last_bounce_order: no scene"; return RPT_EINVAL; }
    const bool on = c->scene.lds_scene != 0u && c->stack_cap == 16 && c->scene.last_emit_n <= RPT_LAST_EMIT_MAX;
    if (mode_out) *mode_out = !on ? 0u : 1u + (uint32_t)c->last_order.rule;
    if (n_emissive_out) *n_emissive_out = c->scene.last_emit_n;
    if (visits_out) for (int k = 0; k < 4; ++k) visits_out[k] = c->last_order.visits[k];
    if (probe_rays_out) *probe_rays_out = c->last_order.probe_rays;
    if (probe_ms_out) *probe_ms_out = c->last_order.probe_ms;
    return RPT_OK;
}

/* the host probes walk the pool: the same validation rpt_upload_scene applies first (a child link that points at an ancestor would never end) */
static int validate_for_host_probe(const rpt_per_vertex_data *pv, size_t nv, const rpt_triangle *idx, size_t nt, const rpt_bvh_node *nodes, size_t nn,
                                   const rpt_material_data *mats, size_t nm, const rpt_light_pick_entry *lp, size_t nlp) {
    rpt_ctx scratch;
    uint32_t depth = 0;
    const int rc = validate_scene(&scratch, pv, nv, idx, nt, nodes, nn, mats, nm, lp, nlp, depth);
    if (rc) rpt_create_error() = scratch.error;
    return rc;
}

/* the reason of this thread's last rpt_debug_shadow_order_host decision (a string literal of shadow_order.h) */
static const char *&host_shadow_why() {
    static thread_local const char *why = "";
    return why;
}

int rpt_debug_shadow_order_host(const rpt_per_vertex_data *pv, size_t nv, const rpt_triangle *idx, size_t nt, const rpt_bvh_node *nodes, size_t nn,
                                const rpt_material_data *mats, size_t nm, const rpt_light_pick_entry *lp, size_t nlp, uint32_t *fixed_out,
                                double *visits_near_out, double *visits_fixed_out, uint32_t *probe_rays_out, uint8_t *flip_out /* (nn - 1) / 2, nullable */) {
    if (!pv || !idx || !nodes || !mats || !lp || nn == 0) return RPT_EINVAL;
    RPT_TRY(validate_for_host_probe(pv, nv, idx, nt, nodes, nn, mats, nm, lp, nlp));
    const bool pair_shaped = pool_is_pair_shaped(nodes, nn);
    const ShadowOrder so = choose_shadow_order(pv, idx, nt, nodes, nn, mats, lp, nlp, pair_shaped, nullptr, rpt_read_knobs().shadow_order);
    if (fixed_out) *fixed_out = so.fixed ? 1u : 0u;
    if (visits_near_out) *visits_near_out = so.visits_near;
    if (visits_fixed_out) *visits_fixed_out = so.visits_fixed;
    if (probe_rays_out) *probe_rays_out = so.probe_rays;
    if (flip_out && !so.flip.empty()) memcpy(flip_out, so.flip.data(), so.flip.size());
    host_shadow_why() = so.why;
    return RPT_OK;
}

const char *rpt_debug_shadow_order_why(rpt_ctx *c) {
    if (!c) return host_shadow_why();
    return c->has_scene ? c->shadow_order.why : "";
}

int rpt_debug_last_order_host(const rpt_per_vertex_data *pv, size_t nv, const rpt_triangle *idx, size_t nt, const rpt_bvh_node *nodes, size_t nn,
                              const rpt_material_data *mats, size_t nm, uint32_t *rule_out, double *visits_out /* [4] */, uint32_t *probe_rays_out,
                              uint8_t *flip_out /* (nn - 1) / 2, nullable */) {
    if (!pv || !idx || !nodes || !mats || nn == 0) return RPT_EINVAL;
    rpt_light_pick_entry none{};
    none.ratio = -1.0f;
    RPT_TRY(validate_for_host_probe(pv, nv, idx, nt, nodes, nn, mats, nm, &none, 1));
    const bool pair_shaped = pool_is_pair_shaped(nodes, nn);
    const LastOrder lo = choose_last_order(pv, idx, nt, nodes, nn, mats, pair_shaped, rpt_read_knobs().last_order);
    if (rule_out) *rule_out = (uint32_t)lo.rule;
    if (visits_out) for (int k = 0; k < 4; ++k) visits_out[k] = lo.visits[k];
    if (probe_rays_out) *probe_rays_out = lo.probe_rays;
    if (flip_out && !lo.flip.empty()) memcpy(flip_out, lo.flip.data(), lo.flip.size());
    return RPT_OK;
}

}  // extern "C"
