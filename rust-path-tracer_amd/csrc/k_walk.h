/*
 * k_walk.h — everything ONE ray needs to walk the BVH (the file header of k_traverse.h says what the walk must reproduce): the stack types, the hit record,
 * the slab tests, the three views of the scene, the triangle test, and the walk loops with their one-shot forms (traverse_loop*, traverse_one).
 */
#ifndef RPT_K_WALK_H
#define RPT_K_WALK_H

#include <type_traits>

#include "k_common.h"
#include "rpt_fastdiv.h"

template <bool SMALL> struct StackElem { typedef uint32_t type; };      /* node indices on the stack */
template <> struct StackElem<true> { typedef uint16_t type; };          /* < 65 536 nodes (and every LDS-resident scene) */
/* The stack of a lane is a column of an LDS array, [entry][lane].  Entry widths: 16 bits (< 65 536 nodes and every
 * LDS-resident scene), 32 bits, and — for the streamed global-memory walks, whose occupancy the LDS footprint caps once
 * indices need more than 16 bits — 24 bits as a 16-bit and an 8-bit column (< 2^24 nodes): 32 entries cost a wave 6 KB
 * instead of 8 KB, 5.5 instead of 4.25 waves per SIMD fit beside each other. */
template <typename T> __device__ __forceinline__ void stack_put(T *s, int sp, uint32_t v) { s[sp * RPT_WAVE] = (T)v; }
template <typename T> __device__ __forceinline__ uint32_t stack_get(T *s, int sp) { return (uint32_t)s[sp * RPT_WAVE]; }
struct Stack24 {
    uint16_t *lo;
    uint8_t *hi;
};
__device__ __forceinline__ void stack_put(Stack24 s, int sp, uint32_t v) {
    s.lo[sp * RPT_WAVE] = (uint16_t)v;
    s.hi[sp * RPT_WAVE] = (uint8_t)(v >> 16);
}
__device__ __forceinline__ uint32_t stack_get(Stack24 s, int sp) { return (uint32_t)s.lo[sp * RPT_WAVE] | ((uint32_t)s.hi[sp * RPT_WAVE] << 16); }
/* 16 + K bits per entry at the LDS cost of 16: the low half in the 16-bit column, bit 16 + k of level sp in bit sp of a per-lane
 * mask register (stacks have at most 32 levels).  One LDS operation per push / pop like the 16-bit stack, a few VALU
 * instructions per extra bit instead of the second column's LDS operation and its 1.5 KB per wave. */
template <int K> struct StackBits {
    uint16_t *lo;
    uint32_t hi[K];
};
template <int K> __device__ __forceinline__ void stack_put(StackBits<K> &s, int sp, uint32_t v) {
    s.lo[sp * RPT_WAVE] = (uint16_t)v;
    const uint32_t keep = ~(1u << sp);
#pragma unroll
    for (int k = 0; k < K; ++k) s.hi[k] = (s.hi[k] & keep) | (((v >> (16 + k)) & 1u) << sp);
}
template <int K> __device__ __forceinline__ uint32_t stack_get(const StackBits<K> &s, int sp) {
    uint32_t v = (uint32_t)s.lo[sp * RPT_WAVE];
#pragma unroll
    for (int k = 0; k < K; ++k) v |= ((s.hi[k] >> sp) & 1u) << (16 + k);
    return v;
}
/* the LDS arrays of one wave's stack for an entry width, and the handle walk_run takes */
template <int STACK, int WIDTH> struct WaveStack {                       /* WIDTH 16 / 32 */
    typedef typename StackElem<WIDTH == 16>::type T;
    T cells[STACK][RPT_WAVE];
    __device__ __forceinline__ T *column(uint32_t lane) { return &cells[0][lane]; }
};
template <int STACK> struct WaveStack<STACK, 21> {                      /* < 2^21 nodes: 16 bits in LDS + 5 mask registers */
    static_assert(STACK <= 32, "one mask bit per stack level");
    uint16_t lo[STACK][RPT_WAVE];
    __device__ __forceinline__ StackBits<5> column(uint32_t lane) { return StackBits<5>{&lo[0][lane], {0u, 0u, 0u, 0u, 0u}}; }
};
template <int STACK> struct WaveStack<STACK, 24> {
    uint16_t lo[STACK][RPT_WAVE];
    uint8_t hi[STACK][RPT_WAVE];
    __device__ __forceinline__ Stack24 column(uint32_t lane) { return Stack24{&lo[0][lane], &hi[0][lane]}; }
};

struct HitRecord {
    float t;
    uint32_t tri;     /* HIT_MISS or triangle index | backface << 31 */
};
/* what the traversal stage leaves in a slot: the 8 bytes the shade stage reads */
__device__ __forceinline__ void store_hit(const DevState &st, uint32_t slot, const HitRecord &r) { st.hit[slot] = make_float2(r.t, __uint_as_float(r.tri)); }

/* the interval a ray spends inside a box from its six plane quotients, in the reference's order of NaN-ignoring min / max (intersection.rs:108-117) */
__device__ __forceinline__ void slab_interval(float tx1, float tx2, float ty1, float ty2, float tz1, float tz2, float &tmin, float &tmax) {
    tmin = rptm::fminr(tx1, tx2);
    tmax = rptm::fmaxr(tx1, tx2);
    tmin = rptm::fmaxr(tmin, rptm::fminr(ty1, ty2));
    tmax = rptm::fminr(tmax, rptm::fmaxr(ty1, ty2));
    tmin = rptm::fmaxr(tmin, rptm::fminr(tz1, tz2));
    tmax = rptm::fminr(tmax, rptm::fmaxr(tz1, tz2));
}
/* intersection.rs:104-122 — NaN-ignoring min/max, strict comparisons as written.  The reference returns
 * tmin or +inf; callers only ever compare that value, so it is kept as (hit, tmin): a hit has a non-NaN
 * tmin < prev_min_t < inf, and "dl > dr" on the inf-encoded values (intersection.rs:216) is
 * hit_r && (!hit_l || tmin_l > tmin_r) — predicates that stay in scalar mask registers. */
template <bool FAST>
__device__ __forceinline__ bool slab_test(float4 lo, float4 hi, F3 ro, F3 rd, F3 ird, float prev_min_t, float &tmin_out) {
    float tx1, tx2, ty1, ty2, tz1, tz2;
    if (FAST) {
        tx1 = rptm::div_by_rcp(lo.x - ro.x, rd.x, ird.x); tx2 = rptm::div_by_rcp(hi.x - ro.x, rd.x, ird.x);
        ty1 = rptm::div_by_rcp(lo.y - ro.y, rd.y, ird.y); ty2 = rptm::div_by_rcp(hi.y - ro.y, rd.y, ird.y);
        tz1 = rptm::div_by_rcp(lo.z - ro.z, rd.z, ird.z); tz2 = rptm::div_by_rcp(hi.z - ro.z, rd.z, ird.z);
    } else {
        tx1 = (lo.x - ro.x) / rd.x; tx2 = (hi.x - ro.x) / rd.x;
        ty1 = (lo.y - ro.y) / rd.y; ty2 = (hi.y - ro.y) / rd.y;
        tz1 = (lo.z - ro.z) / rd.z; tz2 = (hi.z - ro.z) / rd.z;
    }
    float tmin, tmax;
    slab_interval(tx1, tx2, ty1, ty2, tz1, tz2, tmin, tmax);
    tmin_out = tmin;
    return tmax >= tmin && tmax > 0.0f && tmin < prev_min_t;
}

/* the packed 36-byte (e1, e2, a) triangle records, as both global-memory views read them */
struct TriRecords {
    const float *tri_isect;
    __device__ __forceinline__ void edges(uint32_t ti, F3 &e1, F3 &e2) const {
        const float *p = tri_isect + 9u * (size_t)ti;
        e1 = f3(p[0], p[1], p[2]); e2 = f3(p[3], p[4], p[5]);
    }
    __device__ __forceinline__ F3 corner(uint32_t ti) const {
        const float *p = tri_isect + 9u * (size_t)ti + 6u;
        return f3(p[0], p[1], p[2]);
    }
};

/* How the generic loop reads the scene: the uploaded node array as is (children adjacent, one visit = 64
 * contiguous bytes = half a cache line through L1/L2) and the (a, e1, e2) triangle records.  A finished lane
 * carries count = 0x80000000 so that "at an inner node" / "at a leaf" are single compares on the register (a
 * ballot of a compare is the compare itself; a ballot of a loop-carried bool costs two more VALU instructions).
 * Only the one-ray-per-lane walks (a foreign builder's node pool, the test hook) read the scene this way. */
struct SceneViewGlobal : TriRecords {
    static constexpr bool kCoopLeaves = true;               /* leaves may hold dozens of triangles: see walk_run */
    static constexpr bool kUniformScalar = false;
    const float4 *nodes;
    typedef uint2 Cur;                                      /* x = triangle_count, y = left child / first triangle */
    __device__ __forceinline__ Cur root() const { return make_uint2(__float_as_uint(nodes[0].w), __float_as_uint(nodes[1].w)); }
    __device__ __forceinline__ static bool is_inner(Cur c) { return c.x == 0u; }
    __device__ __forceinline__ static bool is_leaf(Cur c) { return (int32_t)c.x > 0; }
    __device__ __forceinline__ static Cur dead() { return make_uint2(0x80000000u, 0u); }
    __device__ __forceinline__ static bool is_dead(Cur c) { return !is_inner(c) && !is_leaf(c); }
    __device__ __forceinline__ static uint32_t leaf_count(Cur c) { return c.x; }
    __device__ __forceinline__ static uint32_t leaf_first(Cur c) { return c.y; }
    __device__ __forceinline__ void children(Cur c, float4 &lmin, float4 &lmax, float4 &rmin, float4 &rmax) const {
        const float4 *ch = nodes + 2u * c.y;
        lmin = ch[0]; lmax = ch[1]; rmin = ch[2]; rmax = ch[3];
    }
    __device__ __forceinline__ static Cur enter(bool right, float4 lmin, float4 lmax, float4 rmin, float4 rmax) {
        return make_uint2(__float_as_uint(right ? rmin.w : lmin.w), __float_as_uint(right ? rmax.w : lmax.w));
    }
    __device__ __forceinline__ uint32_t far_entry(Cur c, bool far_is_left) const { return far_is_left ? c.y : c.y + 1u; }
    __device__ __forceinline__ Cur from_entry(uint32_t e) const {
        return make_uint2(__float_as_uint(nodes[2u * e].w), __float_as_uint(nodes[2u * e + 1u].w));
    }
};

/* The streamed global-memory walks read a PAIR array instead (round 4).  Counters first (profiles/r04_*_pmc_ta.txt): these walks keep the CU's
 * texture-address unit busy 83-92 % of the time (TA_TA_BUSY / TCP_GATE_EN1: VeachMIS shadow 92 %, PBRTest nearest 91 %; the LDS walk 12 %) — that
 * front end is what bounds them.  What a load costs it (tools/microbench/ta_rates.hip, profiles/r04_ta_rates.txt): ~0.5 cycles per LIVE lane and
 * ~10 per instruction whatever the width when the lanes diverge, the data return (64 bytes per clock) on top where lanes share lines.  A visit was
 * four 16-byte loads per lane — the two 32-byte nodes as uploaded, 48 bytes of boxes and 16 of (count, child / first) words.  Here a child pair is
 * ONE 64-byte-aligned record
 *     q0 = (L.lo.xyz, L.hi.x)  q1 = (L.hi.yz, R.lo.xy)  q2 = (R.lo.z, R.hi.xyz)  [8 bytes unused]  (link L, link R)
 * with link = triangle_count << 24 | left child / first triangle: three 16-byte loads and one 8-byte load (still four instructions: boxes are 48
 * bytes; the 8-byte one returns half the data on the shared lines near the top of the tree), and a popped node index costs one 4-byte load from
 * `links[]` instead of two.  Pair p = the children (2p + 1, 2p + 2) of the reference's node pool (its builder allocates children in pairs after the
 * root); a scene whose pool is not pair-shaped, or with a leaf of 255+ triangles or 2^24+ triangles, keeps the one-shot generic walks.  The node
 * is one register: an inner node is its left child's index (< 2^24 - 1: the right child's index, which the walks push, is below 2^24 as well —
 * rpt_scene.hip pool_is_pair_shaped; a pool with a child at 2^24 or beyond keeps the generic walks and their 32-bit entries). */
template <bool COOP>
struct SceneViewPairsT : TriRecords {
    static constexpr bool kCoopLeaves = COOP;                  /* leaves may hold dozens of triangles: see walk_run.  The streamed walks are
                                                                  built both ways and the host picks by the scene's largest leaf: the cooperative
                                                                  leaf code costs registers the walk of a thin-leaf scene (every shipped one) needs */
    const float4 *pairs;          /* 64 bytes per pair: 3 x float4 of boxes, 8 bytes unused, (link L, link R) in the LAST 8 bytes — at offset 48, 16-byte aligned,
                                     the compiler widens the 8-byte load to a 16-byte one; in an array of their own the links cost large scenes a second line */
    const uint32_t *links;        /* per NODE: what a popped stack entry (a node index) resolves to */
    typedef uint32_t Cur;
    __device__ __forceinline__ Cur root() const { return links[0]; }
    __device__ __forceinline__ static bool is_inner(Cur c) { return c < (1u << 24); }
    __device__ __forceinline__ static bool is_leaf(Cur c) { return c + 1u > (1u << 24); }          /* (the dead word wraps to 0) */
    __device__ __forceinline__ static Cur dead() { return 0xffffffffu; }
    __device__ __forceinline__ static bool is_dead(Cur c) { return !is_inner(c) && !is_leaf(c); }
    __device__ __forceinline__ static uint32_t leaf_count(Cur c) { return c >> 24; }
    __device__ __forceinline__ static uint32_t leaf_first(Cur c) { return c & 0xffffffu; }
    __device__ __forceinline__ void children(Cur c, float4 &lmin, float4 &lmax, float4 &rmin, float4 &rmax) const {
        const float4 *p = pairs + 4u * (c >> 1);
        const float4 q0 = p[0], q1 = p[1], q2 = p[2];
        uint2 lk = *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(p) + 56);
        asm volatile("" : "+v"(lk.x), "+v"(lk.y));      /* issued WITH the boxes: left alone the compiler sinks this load behind the slab tests, a second round trip */
        lmin = make_float4(q0.x, q0.y, q0.z, __uint_as_float(lk.x));
        lmax = make_float4(q0.w, q1.x, q1.y, 0.0f);
        rmin = make_float4(q1.z, q1.w, q2.x, __uint_as_float(lk.y));
        rmax = make_float4(q2.y, q2.z, q2.w, 0.0f);
    }
    /* The same record through the SCALAR cache, for a node every participating lane stands on (c is wave-uniform): one s_load_dwordx16 instead
     * of four vector loads — no texture-address cycles at all.  A wave of the first iteration is an 8 x 8 pixel block at one sample index, and at
     * the BASELINE resolutions its 64 camera rays walk the same nodes: 98 % of the inner steps of primary-ray waves are wave-uniform on PBRTest
     * 2048^2 and VeachMIS 1080p (tools/uniform_visit_share.py, profiles/r04_uniform_visit_share.txt).  The wait is inside the asm statement: the
     * compiler's s_waitcnt insertion does not see a load it did not emit.  Destinations are early-clobber ("=&s"): an SMEM destination that overlapped
     * its own base pair would be re-read clobbered if the load were ever replayed (XNACK) — LLVM does the same for its own scalar loads on xnack-any
     * targets. */
    static constexpr bool kUniformScalar = true;
    __device__ __forceinline__ void children_uniform(uint32_t c, float4 &lmin, float4 &lmax, float4 &rmin, float4 &rmax) const {
        typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
        const float4 *p = pairs + 4u * (c >> 1);
        u32x16 r;
        asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(p) : "memory");
        lmin = make_float4(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]), __uint_as_float(r[14]));
        lmax = make_float4(__uint_as_float(r[3]), __uint_as_float(r[4]), __uint_as_float(r[5]), 0.0f);
        rmin = make_float4(__uint_as_float(r[6]), __uint_as_float(r[7]), __uint_as_float(r[8]), __uint_as_float(r[15]));
        rmax = make_float4(__uint_as_float(r[9]), __uint_as_float(r[10]), __uint_as_float(r[11]), 0.0f);
    }
    __device__ __forceinline__ static Cur enter(bool right, float4 lmin, float4, float4 rmin, float4) { return __float_as_uint(right ? rmin.w : lmin.w); }
    __device__ __forceinline__ uint32_t far_entry(Cur c, bool far_is_left) const { return far_is_left ? c : c + 1u; }
    __device__ __forceinline__ Cur from_entry(uint32_t e) const { return links[e]; }
    /* the same for a wave-uniform popped index / a wave-uniform triangle: scalar cache */
    __device__ __forceinline__ Cur from_entry_uniform(uint32_t e) const {
        uint32_t r;
        asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r) : "s"(links + e) : "memory");
        return r;
    }
    __device__ __forceinline__ void triangle_uniform(uint32_t ti, F3 &e1, F3 &e2, F3 &a) const {
        typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
        const float *p = tri_isect + 9u * (size_t)ti;
        u32x8 r;
        uint32_t r8;
        asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dword %1, %2, 0x20\n\ts_waitcnt lgkmcnt(0)" : "=&s"(r), "=&s"(r8) : "s"(p) : "memory");
        e1 = f3(__uint_as_float(r[0]), __uint_as_float(r[1]), __uint_as_float(r[2]));
        e2 = f3(__uint_as_float(r[3]), __uint_as_float(r[4]), __uint_as_float(r[5]));
        a = f3(__uint_as_float(r[6]), __uint_as_float(r[7]), __uint_as_float(r8));
    }
};

/* The LDS-resident image of a small scene, built once at upload (rpt_scene.hip, build_lds_image) and copied into
 * LDS by every workgroup.  Measured on MI355X (tools/microbench/valu_rates.hip, SQ counters in profiles/): the
 * traversal kernel is VALU-ISSUE bound — fma/mul/add issue in ~2 cycles per wave64 instruction, everything else
 * (min/max, compares, selects, integer/address ops) in ~4 — so the image is laid out to delete instructions:
 *
 *   plane records   K_A[p] = (L.lo.k, R.lo.k, L.hi.k, R.hi.k),  K_B[p] = (L.hi.k, R.hi.k, L.lo.k, R.lo.k)
 *                   for axis k = x, y, z and child pair p = nodes (2p+1, 2p+2).  A ray whose direction component is
 *                   positive reads K_A, a negative one K_B (a per-ray base address), so the register quad is always
 *                   (L.near, R.near, L.far, R.far): with lo <= hi and a finite non-zero divisor, RN((lo-o)/d) and
 *                   RN((hi-o)/d) are ordered by the sign of d (RN subtraction and division are monotone), so the
 *                   reference's six f32::min/max per box (intersection.rs:108-117) become one max3 and one min3,
 *                   value for value.  Rays outside the exact-division guard keep the explicit min/max on K_A.
 *   descriptors     D[p] = desc(L) | desc(R) << 16;  desc = 4 x pair index (< 0x4000) of an inner child — the byte offset of
 *                   D[p], a quarter of that of the pair's plane records (lds_at) —,
 *                   0x8000 | triangle_count << 9 | first_triangle for a leaf; 0x4000 marks a finished lane.
 *                   The 16-bit stack holds descriptors, so a pop is one ds_read_u16 — no node lookup.
 *   triangles       (a, e1, e2)[t]  (three 16-byte vectors per triangle, one after the other: one address register
 *                   and immediate offsets serve the three loads of a triangle test)
 *
 * Every load instruction of a node visit addresses "array base + 16 * p": the 16 lanes that ds_read_b128 serves per
 * LDS cycle spread over all 64 banks instead of the 4 bank groups an array-of-nodes layout allows.
 * A node array that is not pair-shaped, has an empty/inverted box, or a leaf of 64+ triangles gets no image and
 * is traversed from global memory by the generic loop. */
struct SceneViewLds {
    static constexpr bool kCoopLeaves = false;
    const float4 *img;
    uint32_t pairs, tris, root_desc;
    typedef uint32_t Cur;                                   /* a 16-bit child descriptor */
    __device__ __forceinline__ Cur root() const { return root_desc; }
    __device__ __forceinline__ static bool is_inner(Cur c) { return c < LDS_DESC_DEAD; }
    __device__ __forceinline__ static bool is_leaf(Cur c) { return c >= LDS_DESC_LEAF; }
    __device__ __forceinline__ static Cur dead() { return LDS_DESC_DEAD; }
    __device__ __forceinline__ static bool is_dead(Cur c) { return c == LDS_DESC_DEAD; }      /* (as the two range tests of the other views the streamed kernels compile to other code) */
    __device__ __forceinline__ const float4 *tri_base() const { return img + 6u * pairs + ((pairs + 3u) >> 2); }
    __device__ __forceinline__ void edges(uint32_t ti, F3 &e1, F3 &e2) const {
        const float4 *t = tri_base() + 3u * ti;
        e1 = xyz4(t[1]); e2 = xyz4(t[2]);
    }
    __device__ __forceinline__ F3 corner(uint32_t ti) const { return xyz4(tri_base()[3u * ti]); }
};
/* what lies `bytes` behind an array of the image: an inner descriptor is its pair index times FOUR, so the pair's descriptor word is at `descs + cur` and
 * its plane records are at `base + (cur << 2)` — one shift-and-add per load, nothing to scale first */
template <typename T> __device__ __forceinline__ T lds_at(const float4 *base, uint32_t bytes) {
    return *reinterpret_cast<const T *>(reinterpret_cast<const char *>(base) + bytes);
}
/* the plane record of the pair behind inner descriptor `desc` in the per-ray array `base`: base + (desc << 2) as ONE instruction (left to itself the compiler
 * shares the shift between the three axes: four instructions for three addresses) */
__device__ __forceinline__ float4 lds_planes(const float4 *base, uint32_t desc) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(3))) float4 *LdsVec;
    const uint32_t b = (uint32_t)(LdsVec)base;
    uint32_t a;
    asm("v_lshl_add_u32 %0, %1, 2, %2" : "=v"(a) : "v"(desc), "v"(b));
    return *(LdsVec)a;
#else
    return lds_at<float4>(base, desc << 2);      /* (the host pass only parses device code) */
#endif
}
/* The lane's stack column by its 32-bit LDS address: the walk keeps the ADDRESS of the next free entry instead of its index, a push is a store and an add, a
 * pop an add and a load (the index costs a shift-and-add at each) */
constexpr uint32_t LDS_STACK_STRIDE = RPT_WAVE * (uint32_t)sizeof(uint16_t);      /* bytes from one entry of a column to the next */
__device__ __forceinline__ uint32_t lds_stack_address(const uint16_t *stack) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)(const __attribute__((address_space(3))) uint16_t *)stack;
#else
    return 0u;
#endif
}
__device__ __forceinline__ void lds_stack_store(uint32_t at, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *(__attribute__((address_space(3))) uint16_t *)at = (uint16_t)v;
#endif
}
__device__ __forceinline__ uint32_t lds_stack_load(uint32_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const __attribute__((address_space(3))) uint16_t *)at;
#else
    return 0u;
#endif
}

/* intersection.rs:9-54 with edge1/edge2 precomputed at upload; `corner` is a callable: it is asked for the corner only by lanes that get
 * past the determinant test */
template <typename Corner>
__device__ __forceinline__ bool moller_trumbore(F3 edge1, F3 edge2, Corner corner, F3 ro, F3 rd, float &out_t, bool &backface) {
    F3 pv = cross3(rd, edge2);
    float det = dot3(edge1, pv);
    backface = (rptm::f2u(det) >> 31) != 0u;
    if (rptm::absr(det) < 1e-6f) return false;
    float inv_det = rptm::rcp_rn(det);
    F3 tv = ro - corner();
    float u = dot3(tv, pv) * inv_det;
    if (u < 0.0f || u > 1.0f) return false;
    F3 qv = cross3(tv, edge1);
    float v = dot3(rd, qv) * inv_det;
    if (v < 0.0f || u + v > 1.0f) return false;
    float t = dot3(edge2, qv) * inv_det;
    if (t < 0.0f) return false;
    out_t = t;
    return true;
}
template <typename View>
__device__ __forceinline__ bool moller_trumbore_view(const View &view, uint32_t ti, F3 ro, F3 rd, float &out_t, bool &backface) {
    F3 edge1, edge2;
    view.edges(ti, edge1, edge2);
    return moller_trumbore(edge1, edge2, [&] { return view.corner(ti); }, ro, rd, out_t, backface);
}
/* the same test on a record the caller already holds in registers (the wave-cooperative leaves load a leaf once for all the
 * lanes that wait at it) */
__device__ __forceinline__ bool moller_trumbore_regs(F3 edge1, F3 edge2, F3 corner, F3 ro, F3 rd, float &out_t, bool &backface) {
    return moller_trumbore(edge1, edge2, [&] { return corner; }, ro, rd, out_t, backface);
}

/* One ray per lane through the BVH.  Per lane the sequence of box tests, triangle tests and the value of the
 * running best t at each of them is exactly the reference's (intersection.rs:177-234); what is scheduled is
 * WHEN a lane takes its next step.  Each trip of the loop the wave issues ONE body, the one with more lanes ready
 * for it: the box step for the lanes standing on an inner node, or the triangle body for the lanes standing on a leaf
 * (a tie goes to the box step).
 * Why: after the first bounce the rays of a wave are incoherent.  A replay of the reference traversal on real
 * DarkCornell bounce rays (tools/traversal_sim.py) gives, in issue slots per ray: classic while-while 148
 * (lanes at a leaf wait for the slowest lane of every round), one-step-per-trip "if-if" 113 (the leaf body,
 * 14 % of the steps, is issued on almost every trip), deferred leaves (wait for K lanes at a leaf) with K = 12..16: 106; ideal 38.
 * Measured on MI355X the gain is smaller (LDS/latency share the bill with VALU issue): traverse 23.7 -> 22.4..22.8 ms for
 * K = 8..16, 25.9 ms for K = 64 (= while-while).  The one-body rule then beat the K = 8 threshold on the global-memory walks
 * (K = 8 / one body / a leaf counting 60 % of an inner step: VeachMIS 5175 / 5506 / 5453 Mrays/s, PBRTest 4915 / 5027 / 5011).
 * `stack` points at this lane's column of the wave's LDS stack: entry e lives at stack[e * RPT_WAVE]. */
__device__ __forceinline__ float rpt_readlane(float v, int lane) { return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), lane)); }
__device__ __forceinline__ uint32_t rpt_readlane_u(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }

/* every active lane holds x0 in x (x0: wave-uniform, the readfirstlane of x — taken by the caller: handed back by this helper, the any-hit and the
 * fat-leaf global-memory walks compile to other code) */
__device__ __forceinline__ bool rpt_all_lanes_hold(uint32_t x, uint32_t x0) { return rpt_ballot(x == x0) == rpt_ballot(true); }

/* Everything a ray needs besides (ro, rd, 1/rd) and its stack column: the walk can be stopped after a number of loop
 * trips and resumed (the streamed kernels hand finished lanes new rays in between). */
template <typename View> struct Walk {
    typename View::Cur cur;    /* node the ray stands on; View::dead() when finished / no ray */
    int sp;
    HitRecord res;
};
template <typename View>
__device__ __forceinline__ void walk_begin(const View &view, Walk<View> &w) {
    w.cur = view.root();
    w.sp = 0;
    w.res.t = 1000000.0f;
    w.res.tri = HIT_MISS;
}
template <typename View>
__device__ __forceinline__ bool walk_dead(const Walk<View> &w) { return View::is_dead(w.cur); }

/* At most `budget` trips of the deferred-leaf loop for the lanes of this wave; returns early when no lane has anything
 * left.  Per ray the visiting order and every comparison are the reference's. */
/* the node behind a popped stack entry; a wave-uniform entry (coherent camera rays pop together) comes through the scalar cache */
template <bool ANY_HIT, typename View>
__device__ __forceinline__ typename View::Cur walk_pop(const View &view, uint32_t e) {
    if constexpr (View::kUniformScalar && !ANY_HIT && !View::kCoopLeaves) {      /* (measured: + 1.5 % PBRTest, + 0.6 % VeachMIS; nothing on any-hit walks and on the fat-leaf build) */
        const uint32_t e0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
        if (rpt_all_lanes_hold(e, e0)) return view.from_entry_uniform(e0);
        asm volatile("" ::: "memory");
        return view.from_entry(e);
    } else {
        return view.from_entry(e);
    }
}

/* RPT_SHADOW_SEGMENT (rpt.h rpt_set_shadow_mode), the opt-in any-hit walk that is NOT the reference's: a child box is entered iff the reference's test
 * passes AND tmin <= max_t — a shadow ray is a segment, and only triangles with t <= max_t can be accepted, so boxes that begin behind the light point
 * are left out.  The SEGMENT instantiations of the walks take this bound in the place of max_t: the value every t of the ray is compared against,
 *     tmin <= max_t  <=>  tmin < bound     and     t < 1e6 && t <= max_t  <=>  t < bound
 * (bound = the float after max_t, or 1e6 from max_t = 1e6 on, where the mode is the reference's walk; a NaN max_t stays NaN: nothing passes, as nothing
 * passes t <= NaN).  result.t is 1e6 until the first accept and the walk ends there (intersection.rs:191-203), so the bound takes the place of the
 * constant the slab test compares tmin against and of both comparisons of the triangle test: the bounded step has no instruction the exact one lacks. */
__device__ __forceinline__ float shadow_segment_bound(float max_t) {
    if (!(max_t < 1000000.0f)) return max_t >= 1000000.0f ? 1000000.0f : max_t;
    if (max_t == 0.0f) return __uint_as_float(1u);
    const uint32_t b = __float_as_uint(max_t);
    return __uint_as_float(max_t > 0.0f ? b + 1u : b - 1u);
}

template <int STACK, bool ANY_HIT, bool FAST, bool FIXED = false, bool SEGMENT = false /* max_t holds shadow_segment_bound(max_t) */, typename View, typename StackRef>
__device__ __forceinline__ void walk_run(const View &view, Walk<View> &w, F3 ro, F3 rd, F3 ird, float max_t, StackRef &stack, int budget) {
    static_assert(!FIXED || ANY_HIT, "only the any-hit walk may choose its order");
    static_assert(!SEGMENT || ANY_HIT, "only a shadow ray is a segment");
    typedef typename View::Cur Cur;
    HitRecord res = w.res;
    int sp = w.sp;
    Cur cur = w.cur;
    for (int trip = 0; trip < budget; ++trip) {
        const bool at_inner = View::is_inner(cur);
        const bool at_leaf = View::is_leaf(cur);
        const unsigned long long inner_m = rpt_ballot(at_inner), leaf_m = rpt_ballot(at_leaf);
        if ((inner_m | leaf_m) == 0ull) break;
        /* one body per trip (see above); the rule is written out ahead of each body: evaluated once ahead of both, the same
         * comparison compiles to a different schedule */
        if (at_inner && (uint32_t)__popcll(leaf_m) <= (uint32_t)__popcll(inner_m)) {
            /* inner node (:207-229): test both children against the current best t */
            float4 lmin, lmax, rmin, rmax;
            float tl, tr;
            bool hit_l, hit_r;
            if constexpr (View::kUniformScalar) {
                /* all the lanes of this step on ONE node (a wave of camera rays: nearly always): its record comes through the scalar cache, and the
                 * slab tests read the planes as scalar operands (tested INSIDE the branch: merged behind it, fourteen v_mov would carry them into VGPRs) */
                const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur);
                if (rpt_all_lanes_hold(cur, c0)) {
                    view.children_uniform(c0, lmin, lmax, rmin, rmax);
                    hit_l = slab_test<FAST>(lmin, lmax, ro, rd, ird, SEGMENT ? max_t : res.t, tl);
                    hit_r = slab_test<FAST>(rmin, rmax, ro, rd, ird, SEGMENT ? max_t : res.t, tr);
                    asm volatile("" : "+v"(tl), "+v"(tr));      /* (or the optimiser sinks both branches' tests into ONE copy behind the branch) */
                } else {
                    asm volatile("" ::: "memory");      /* (keeps the four vector loads on THIS side of the branch: hoisted above it they are issued on every step) */
                    view.children(cur, lmin, lmax, rmin, rmax);
                    hit_l = slab_test<FAST>(lmin, lmax, ro, rd, ird, SEGMENT ? max_t : res.t, tl);
                    hit_r = slab_test<FAST>(rmin, rmax, ro, rd, ird, SEGMENT ? max_t : res.t, tr);
                }
            } else {
                view.children(cur, lmin, lmax, rmin, rmax);
                hit_l = slab_test<FAST>(lmin, lmax, ro, rd, ird, SEGMENT ? max_t : res.t, tl);
                hit_r = slab_test<FAST>(rmin, rmax, ro, rd, ird, SEGMENT ? max_t : res.t, tr);
            }
            const bool swap = FIXED ? (hit_r && !hit_l) : (hit_r && (!hit_l || tl > tr));     /* strict: ties keep left first */
            if (hit_l || hit_r) {
                if (hit_l && hit_r && sp < STACK) {
                    stack_put(stack, sp, view.far_entry(cur, swap));
                    sp += 1;
                }
                cur = View::enter(swap, lmin, lmax, rmin, rmax);
            } else if (sp == 0) {
                cur = View::dead();
            } else {
                sp -= 1;
                cur = walk_pop<ANY_HIT>(view, stack_get(stack, sp));
            }
        }
        const bool do_leaf = (uint32_t)__popcll(leaf_m) > (uint32_t)__popcll(inner_m);    /* (wave-uniform) */
        if (do_leaf) {
            bool accepted = false, coop_done = false;
            const uint32_t count = View::leaf_count(cur), first = View::leaf_first(cur);
            if constexpr (View::kCoopLeaves) {
                /* FAT leaves, wave-cooperatively.  The reference's builder stops splitting where the SAH says so, and on
                 * clustered geometry that leaves up to 64 triangles in a leaf (the 1 M-triangle stand-in: 140 triangle
                 * tests per ray).  One lane looping over 64 triangles while the other 63 wait ran that scene at 7 % lane
                 * utilisation (profiles/r02base_deepbvh_pmc_sq.txt).  Instead the owner's ray is broadcast (readlane:
                 * it lives in scalar registers) and every lane tests ONE triangle of the leaf.  The sequential loop
                 * accepts t_i < running best in index order, i.e. ends with the smallest t and, among equal t, the lowest
                 * index (any-hit: the lowest index that passes) — which is what the scalar scan below selects. */
                const bool fat = at_leaf && count > (uint32_t)RPT_COOP_LEAF_MIN;
                unsigned long long todo = rpt_ballot(fat);
                if (todo != 0ull) {
                    const unsigned long long exec_m = rpt_ballot(true);
                    const uint32_t n_act = (uint32_t)__popcll(exec_m);
                    const uint32_t my_rank = rpt_lane_rank(exec_m);
                    coop_done = fat;
                    do {
                        /* ONE load of the leaf's records serves every lane of the wave that waits at this very leaf: a wave is one
                         * 8 x 8 pixel block, so after generation (and for shadow rays towards one light) most of a wave
                         * stands on the same leaf — each used to fetch the 2.3 KB again */
                        const int lead = __ffsll((long long)todo) - 1;
                        const uint32_t b_count = rpt_readlane_u(count, lead), b_first = rpt_readlane_u(first, lead);
                        const unsigned long long group = rpt_ballot(fat && first == b_first && count == b_count) & todo;
                        todo &= ~group;
                        for (uint32_t base = 0; base < b_count; base += n_act) {
                            const bool mine = base + my_rank < b_count;
                            const uint32_t ti = b_first + base + my_rank;
                            F3 e1 = f3(0, 0, 0), e2 = f3(0, 0, 0), corner = f3(0, 0, 0);
                            if (mine) {
                                view.edges(ti, e1, e2);
                                corner = view.corner(ti);
                            }
                            unsigned long long g = ANY_HIT ? (group & ~rpt_ballot(accepted)) : group;
                            while (g != 0ull) {
                                const int L = __ffsll((long long)g) - 1;
                                g &= g - 1ull;
                                const F3 bo = f3(rpt_readlane(ro.x, L), rpt_readlane(ro.y, L), rpt_readlane(ro.z, L));
                                const F3 bd = f3(rpt_readlane(rd.x, L), rpt_readlane(rd.y, L), rpt_readlane(rd.z, L));
                                const float b_max = ANY_HIT ? rpt_readlane(max_t, L) : 0.0f;
                                uint32_t best_bits = __float_as_uint(rpt_readlane(res.t, L));      /* positive floats order like their bits */
                                uint32_t best_tri = HIT_MISS;
                                float t = 0.0f;
                                bool bf = false;
                                const bool acc = mine && moller_trumbore_regs(e1, e2, corner, bo, bd, t, bf) && t > 0.001f &&
                                                 __float_as_uint(t) < best_bits && (!ANY_HIT || (SEGMENT ? t < b_max : t <= b_max));
                                unsigned long long am = rpt_ballot(acc);
                                while (am != 0ull) {                                          /* scalar scan, lowest triangle first */
                                    const int l = __ffsll((long long)am) - 1;
                                    am &= am - 1ull;
                                    const uint32_t tb = __float_as_uint(rpt_readlane(t, l));
                                    if (tb < best_bits) {
                                        best_bits = tb;
                                        best_tri = rpt_readlane_u(ti, l) | (rpt_readlane_u(bf ? 1u : 0u, l) << 31);
                                        if (ANY_HIT) break;
                                    }
                                }
                                if ((int)__lane_id() == L && best_tri != HIT_MISS) {
                                    res.t = __uint_as_float(best_bits);
                                    res.tri = best_tri;
                                    accepted = true;
                                }
                            }
                        }
                    } while (todo != 0ull);
                }
            }
            if (at_leaf && !coop_done) {
                /* leaf triangles in index order (:186-205) */
                bool leaf_uniform = false;
                uint32_t c0 = 0u;
                if constexpr (View::kUniformScalar && !ANY_HIT && !View::kCoopLeaves) {
                    /* every lane of this step on ONE leaf (coherent camera rays): its 36-byte triangle records through the scalar cache */
                    c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur);
                    leaf_uniform = rpt_all_lanes_hold(cur, c0);
                    if (leaf_uniform) {
                        const uint32_t n0 = View::leaf_count(c0), f0 = View::leaf_first(c0);
                        for (uint32_t i = 0; i < n0; ++i) {
                            const uint32_t ti = f0 + i;
                            F3 e1, e2, a;
                            view.triangle_uniform(ti, e1, e2, a);
                            float t = 0.0f;
                            bool bf = false;
                            if (moller_trumbore_regs(e1, e2, a, ro, rd, t, bf) && t > 0.001f && t < res.t) {
                                asm volatile("" ::: "memory");
                                res.t = t;
                                res.tri = ti | (bf ? 0x80000000u : 0u);
                            }
                        }
                    }
                }
                if (!leaf_uniform) {
                asm volatile("" ::: "memory");
                for (uint32_t i = 0; i < count; ++i) {
                    uint32_t ti = first + i;
                    float t = 0.0f;
                    bool bf = false;
                    if (moller_trumbore_view(view, ti, ro, rd, t, bf) && t > 0.001f && (SEGMENT ? t < max_t : (t < res.t && (!ANY_HIT || t <= max_t)))) {
                        /* result.t = result.t.min(t) with t < result.t already established (intersection.rs:195-199).  Kept a
                         * real branch: as two selects on vcc the update becomes back-to-back VOP2 v_cndmask, which gfx950 issues
                         * at ~22 cycles each (tools/microbench/valu_rates.hip) */
                        asm volatile("" ::: "memory");
                        res.t = t;
                        res.tri = ti | (bf ? 0x80000000u : 0u);
                        if (ANY_HIT) { accepted = true; break; }
                    }
                }
                }
            }
            if (at_leaf) {
                if ((ANY_HIT && accepted) || sp == 0) {
                    cur = View::dead();
                } else {
                    sp -= 1;
                    cur = walk_pop<ANY_HIT>(view, stack_get(stack, sp));
                }
            }
        }
    }
    w.cur = cur;
    w.sp = sp;
    w.res = res;
}

/* The same walk over the LDS image (SceneViewLds).  SIGNED = the ray passed the exact-division guard: plane
 * records are read through the per-ray sign-selected bases and near/far need no min/max. */
template <bool SIGNED>
__device__ __forceinline__ bool slab_pair_lds(float n_x, float n_y, float n_z, float f_x, float f_y, float f_z, F3 ro, F3 rd, F3 ird,
                                              float prev_min_t, float &tmin_out) {
    float tmin, tmax;
    if (SIGNED) {
        float a = rptm::div_by_rcp(n_x - ro.x, rd.x, ird.x), b = rptm::div_by_rcp(n_y - ro.y, rd.y, ird.y), c = rptm::div_by_rcp(n_z - ro.z, rd.z, ird.z);
        float d = rptm::div_by_rcp(f_x - ro.x, rd.x, ird.x), e = rptm::div_by_rcp(f_y - ro.y, rd.y, ird.y), f = rptm::div_by_rcp(f_z - ro.z, rd.z, ird.z);
        tmin = __builtin_fmaxf(__builtin_fmaxf(a, b), c);       /* no NaN on this path: plain max3 / min3 */
        tmax = __builtin_fminf(__builtin_fminf(d, e), f);
    } else {
        float tx1 = (n_x - ro.x) / rd.x, tx2 = (f_x - ro.x) / rd.x;
        float ty1 = (n_y - ro.y) / rd.y, ty2 = (f_y - ro.y) / rd.y;
        float tz1 = (n_z - ro.z) / rd.z, tz2 = (f_z - ro.z) / rd.z;
        slab_interval(tx1, tx2, ty1, ty2, tz1, tz2, tmin, tmax);
    }
    tmin_out = tmin;
    return tmax >= tmin && tmax > 0.0f && tmin < prev_min_t;
}

/* The LDS loop schedules its bodies like walk_run: one per trip, the one with more lanes ready.  Its inner step is ~25 % cheaper
 * than the generic one, so the deferred-leaf threshold it had before was higher (one ray per lane: traverse 28.4 ms at K = 8,
 * 26.8-27.3 ms for K = 16..32, 29.0 ms at 48; streamed: 26.0 / 23.7 / 23.5 / 22.6 / 23.3 ms for K = 8 / 12 / 16 / 24 / 32); the
 * one-body rule beat K = 24 and the rules that count a leaf step as more than an inner one (streamed DarkCornell: traverse
 * 82.6 / 80.0 / 81.4 / 82.8 ms per 8 batches for K = 24 / one body / leaf at 130 % / 170 %). */
/* A walk over the LDS image that can be stopped after a number of loop trips and resumed (k_traverse_nearest_stream):
 * everything a ray needs besides (ro, rd, 1/rd) is in here and in its stack column. */
typedef Walk<SceneViewLds> LdsWalk;     /* cur: the descriptor of the node the ray stands on; LDS_DESC_DEAD when finished / no ray */

/* PRESUB (the camera rays of a call's first iteration, k_traverse_nearest_stream FIRST): every ray of the launch has the SAME origin, and the workgroup
 * staged the plane records with that origin already subtracted — the very `plane - ro` (one IEEE subtraction of the same two floats) each lane would
 * compute at each of the twelve planes of a node pair.  The slab test then divides the staged value directly; the triangle test keeps the true origin. */
template <int STACK, bool ANY_HIT, bool SIGNED, bool FIXED = false, bool PRESUB = false, bool SEGMENT = false /* as in walk_run */>
__device__ __forceinline__ void lds_walk_run(const SceneViewLds &view, LdsWalk &w, F3 ro, F3 rd, F3 ird, float max_t, uint16_t *stack, int budget) {
    static_assert(!FIXED || ANY_HIT, "only the any-hit walk may choose its order");
    static_assert(!SEGMENT || ANY_HIT, "only a shadow ray is a segment");
    const F3 ro_slab = PRESUB ? f3(0.0f, 0.0f, 0.0f) : ro;         /* x - (+0) is x, bit for bit: the subtraction folds away */
    const uint32_t P = view.pairs;
    const float4 *img = view.img;
    /* per-ray plane-record bases (float4 units): x | y | z, A or B variant by the sign of the direction */
    const float4 *px = img + ((SIGNED && rd.x < 0.0f) ? P : 0u);
    const float4 *py = img + 2u * P + ((SIGNED && rd.y < 0.0f) ? P : 0u);
    const float4 *pz = img + 4u * P + ((SIGNED && rd.z < 0.0f) ? P : 0u);
    const float4 *descs = img + 6u * P;
    uint32_t cur = w.cur;
    const uint32_t bottom = lds_stack_address(stack), limit = bottom + (uint32_t)STACK * LDS_STACK_STRIDE;
    uint32_t top = bottom + (uint32_t)w.sp;                            /* the next free entry of the lane's column (w.sp of an LDS walk: the stack's height in BYTES of a column) */
    HitRecord res = w.res;
    for (int trip = 0; trip < budget; ++trip) {
        const bool at_inner = SceneViewLds::is_inner(cur);
        const bool at_leaf = SceneViewLds::is_leaf(cur);
        const unsigned long long inner_m = rpt_ballot(at_inner), leaf_m = rpt_ballot(at_leaf);
        if ((inner_m | leaf_m) == 0ull) break;
        /* ONE body per trip, the one with more lanes ready for it: lanes on a leaf no longer sit out a fixed quota of inner
         * steps, and no body is issued for a handful of lanes */
        /* The two counts are pinned to scalar registers: left alone the compiler widens the comparison to 64 bits, which the scalar unit cannot do, and takes it
         * on the vector unit (v_mov + v_cmp_gt_u64 per trip).  Measured on MI355X, DarkCornell 1024^2, traverse per 8 batches: this form 60.4 ms, the vector
         * form 60.4, a wave-uniform branch around the two bodies 60.3 (one more instruction in each pop) — no difference a run can tell; this one has the
         * fewest vector instructions (profiles/r21_walk_overhead_ab.txt).  (Round 3's scalar form, 75.8 -> 77.0 ms, also multiplied one count: a longer chain.) */
        uint32_t n_leaf = (uint32_t)__popcll(leaf_m), n_inner = (uint32_t)__popcll(inner_m);
        asm("" : "+s"(n_leaf), "+s"(n_inner));
        const bool do_leaf = n_leaf > n_inner;
        if (at_inner && !do_leaf) {
            /* (L.near, R.near, L.far, R.far) per axis; without the sign-selected bases (a ray outside the division guard) the three bases are wave-uniform and
             * the compiler's own addresses are the shorter ones */
            const float4 X = SIGNED ? lds_planes(px, cur) : lds_at<float4>(px, cur << 2), Y = SIGNED ? lds_planes(py, cur) : lds_at<float4>(py, cur << 2),
                         Z = SIGNED ? lds_planes(pz, cur) : lds_at<float4>(pz, cur << 2);
            const uint32_t d = lds_at<uint32_t>(descs, cur);
            float tl, tr;
            const bool hit_l = slab_pair_lds<SIGNED>(X.x, Y.x, Z.x, X.z, Y.z, Z.z, ro_slab, rd, ird, SEGMENT ? max_t : res.t, tl);
            const bool hit_r = slab_pair_lds<SIGNED>(X.y, Y.y, Z.y, X.w, Y.w, Z.w, ro_slab, rd, ird, SEGMENT ? max_t : res.t, tr);
            const bool swap = FIXED ? (hit_r && !hit_l) : (hit_r && (!hit_l || tl > tr));     /* strict: ties keep left first */
            if (hit_l || hit_r) {
                const uint32_t nf = __builtin_amdgcn_alignbit(d, d, swap ? 16u : 0u);    /* near | far << 16 */
                if (hit_l && hit_r && top < limit) {
                    lds_stack_store(top, nf >> 16);
                    top += LDS_STACK_STRIDE;
                }
                cur = nf & 0xffffu;
            } else if (top == bottom) {
                cur = LDS_DESC_DEAD;
            } else {
                top -= LDS_STACK_STRIDE;
                cur = lds_stack_load(top);
            }
        }
        if (at_leaf && do_leaf) {
            bool accepted = false;
            const uint32_t count = (cur >> 9) & 63u, first = cur & 511u;
            const float4 *rec = view.tri_base() + 3u * first;      /* (corner, edge1, edge2) of the leaf's triangles, one after the other */
            for (uint32_t ti = first, end = first + count; ti != end; ++ti, rec += 3) {
                float t;                                           /* (read only behind a passed test: set to 0 ahead of it, every early-out costs a v_mov) */
                bool bf = false;
                if (moller_trumbore(xyz4(rec[1]), xyz4(rec[2]), [&] { return xyz4(rec[0]); }, ro, rd, t, bf) && t > 0.001f && (SEGMENT ? t < max_t : (t < res.t && (!ANY_HIT || t <= max_t)))) {
                    /* (a real branch, as in walk_run) */
                    asm volatile("" ::: "memory");
                    res.t = t;
                    res.tri = ti | (bf ? 0x80000000u : 0u);
                    if (ANY_HIT) { accepted = true; break; }
                }
            }
            if ((ANY_HIT && accepted) || top == bottom) {
                cur = LDS_DESC_DEAD;
            } else {
                top -= LDS_STACK_STRIDE;
                cur = lds_stack_load(top);
            }
        }
    }
    w.cur = cur;
    w.sp = (int)(top - bottom);
    w.res = res;
}

/* ---- the walk of the STREAMED LDS kernels (k_traverse_nearest_stream, k_traverse_shadow_stream): lds_walk_run<SIGNED> with its control flattened ----
 * Per lane it computes what lds_walk_run computes, test for test and in the same order; what differs is how the wave is steered.  Every `if` of a lane-varying
 * condition costs the SCALAR unit an exec save, a branch and a restore, plus the mask logic that joins the paths, and a SIMD gets a scalar issue slot only every
 * ~3.5 cycles (profiles/r04_valu_pipes.txt, question 3): on an inner trip of lds_walk_run the scalar port was as long as the vector port.
 *   - the triangle test is moller_trumbore_flat: no early-outs, ONE predicate;
 *   - ONE pop site per trip behind both bodies: a body leaves LDS_DESC_POP in `cur` where the lane has to pop;
 *   - the column's entry 0 holds LDS_DESC_DEAD for good (lds_stream_stack_begin): a pop of an empty stack loads it, there is no `top == bottom` test.  The walk
 *     has STACK - 1 entries; an LDS image has at most 15 levels under its root (rpt_scene.hip stage_nodes), which is what 16-entry columns leave;
 *   - descend / push by selects, the stack store under the only exec narrowing of the inner step;
 *   - the vote is two wave-uniform branches (one scalar shift ahead of them where a lane on a leaf counts double, VOTE), and the loop has ONE exit, at its end: a scalar minimum, a compare and a branch on SCC (an exit at the head, or a
 *     `break` inside, is carried as a lane mask through a latch block). */
/* MIXED (the last extension rays of a batch without NEE, k_traverse_nearest_stream<.., LAST = true>): a nearest-hit walk in which SOME lanes only have to
 * answer "hit or miss" — `stop_first` lanes leave at their first accepted triangle, which is where the reference's walk makes result.hit true for good
 * (intersection.rs:195-203), and because nothing was accepted before, result.t was 1e6 at every box test up to there: the part of the walk they run is an
 * any-hit walk, whose answer does not depend on the visiting order (header).  They read the planes and child descriptors of `img_lane` — the flipped copy
 * of the pair records when the workgroup staged one, then with order_bias = +inf (tl > tr + inf is never true: the left child first, the fixed order of
 * shadow_order.h choose_last_order); the other lanes read the primary image with order_bias = 0 (tr + 0 compares like tr) and are the reference's walk to its end. */
constexpr uint32_t LDS_DESC_POP = LDS_DESC_DEAD + 1u;      /* never in the image, never alive across a trip: neither inner (< DEAD) nor a leaf (>= LEAF) nor dead */
__device__ __forceinline__ void lds_stream_stack_begin(uint16_t *stack) { stack[0] = (uint16_t)LDS_DESC_DEAD; }
__device__ __forceinline__ uint16_t *lds_stream_stack_rest(uint16_t *stack) { return stack + RPT_WAVE; }      /* the STACK - 1 entries above the sentinel, for lds_walk_run */

/* intersection.rs:9-54 for every lane at once: det, u, v and t are computed whatever the earlier tests say, and the four early-outs are one predicate.
 *     u < 0 || v < 0          <=>  fminr(u, v) < 0         (NaN-ignoring min: a NaN operand passes its own test and leaves the other's, as `if (u < 0.0 ..) return` does)
 *     u > 1 || u + v > 1      <=>  fmaxr(u, u + v) > 1     (a NaN u makes u + v NaN: both pass; a NaN v leaves u > 1)
 *     t < 0                        is implied by the caller's t > 0.001, which every accept goes through (a NaN t fails that one)
 * A lane whose |det| < 1e-6 runs the reciprocal like the others (of 0: inf, through rcp_rn's fallback) and is rejected by the predicate. */
__device__ __forceinline__ bool moller_trumbore_flat(F3 edge1, F3 edge2, F3 corner, F3 ro, F3 rd, float &out_t, float &out_det) {
    const F3 pv = cross3(rd, edge2);
    const float det = dot3(edge1, pv);
    const float inv_det = rptm::rcp_rn(det);
    const F3 tv = ro - corner;
    const float u = dot3(tv, pv) * inv_det;
    const F3 qv = cross3(tv, edge1);
    const float v = dot3(rd, qv) * inv_det;
    float lo = rptm::fminr(u, v), hi = rptm::fmaxr(u, u + v), t = dot3(edge2, qv) * inv_det;
    asm volatile("" : "+v"(lo), "+v"(hi), "+v"(t));      /* all three stand in registers HERE: left alone the optimiser turns the predicate back into a ladder of branches */
    out_t = t;
    out_det = det;
    return !(rptm::absr(det) < 1e-6f) & !(lo < 0.0f) & !(hi > 1.0f);
}

/* ONE_TRI and VOTE (the plain nearest-hit kernel).  A leaf trip in which every lane walks its whole leaf runs as long as its longest leaf: on
 * DarkCornell one leaf visit in ten holds a second triangle, a leaf trip carries 20-28 lanes, so nearly every leaf trip ran a second triangle iteration for about
 * three lanes of 64.  With ONE_TRI a leaf trip has no triangle loop: it tests ONE triangle, `cur & 511`, of every lane on a leaf; a lane whose leaf holds more keeps
 * standing on the REST of it, the leaf (first + 1, count - 1) — the descriptor minus LDS_LEAF_REST — and takes its next triangle in the next leaf trip.  Per lane the
 * triangles are tested in the same order against the same res.t; `cur` survives the end of a trip budget and a refill already, and nothing on the stack changes.
 * The rest of a leaf stays a leaf descriptor: its count is never taken below 1 (no borrow into LDS_DESC_LEAF), and first + count <= 512 in every leaf of an image
 * (rpt_scene.hip build_lds_image), so first + 1 stays inside its 9 bits.
 * VOTE is the weight of a lane on a leaf in the vote, as a shift: the leaf trip runs iff (n_leaf << VOTE) > n_inner.  A lane with part of a leaf left idles through the
 * inner trips until the next leaf trip, so one triangle per trip only pays with leaf trips at half the lanes (VOTE = 1; tools/leaf_trip_sim.py). */
constexpr uint32_t LDS_LEAF_REST = (1u << 9) - 1u;                    /* leaf (first, count) - LDS_LEAF_REST = leaf (first + 1, count - 1) */
constexpr uint32_t LDS_DESC_LEAF_MANY = LDS_DESC_LEAF | (2u << 9);    /* a leaf descriptor >= this one holds two triangles or more */
static_assert(LDS_DESC_LEAF == (1u << 15) && LDS_DESC_LEAF_MANY - LDS_LEAF_REST == (LDS_DESC_LEAF | (1u << 9) | 1u), "descriptor = LEAF | count << 9 | first, count in 6 bits");

template <int STACK, bool ANY_HIT, bool FIXED = false, bool MIXED = false, bool PRESUB = false, bool SEGMENT = false /* as in walk_run */, int VOTE = 0, bool ONE_TRI = false>
__device__ __forceinline__ void lds_stream_walk_run(const SceneViewLds &view, LdsWalk &w, F3 ro, F3 rd, F3 ird, float max_t, uint16_t *stack /* entry 0: the sentinel */,
                                                    int budget, const float4 *img_lane = nullptr, uint32_t stop_first = 0u, float order_bias = 0.0f) {
    static_assert(!FIXED || ANY_HIT, "only the any-hit walk may choose its order");
    static_assert(!MIXED || (!ANY_HIT && !FIXED), "MIXED is the nearest-hit walk with per-lane early exits");
    static_assert(!SEGMENT || ANY_HIT, "only a shadow ray is a segment");
    const F3 ro_slab = PRESUB ? f3(0.0f, 0.0f, 0.0f) : ro;
    const uint32_t P = view.pairs;
    const float4 *img = MIXED ? img_lane : view.img;
    const float4 *px = img + (rd.x < 0.0f ? P : 0u);
    const float4 *py = img + 2u * P + (rd.y < 0.0f ? P : 0u);
    const float4 *pz = img + 4u * P + (rd.z < 0.0f ? P : 0u);
    const float4 *descs = img + 6u * P;
    uint32_t cur = w.cur;
    const uint32_t bottom = lds_stack_address(stack) + LDS_STACK_STRIDE, limit = bottom + (uint32_t)(STACK - 1) * LDS_STACK_STRIDE;
    uint32_t top = bottom + (uint32_t)w.sp;                            /* (a lane that popped the sentinel stands one entry BELOW bottom until walk_begin) */
    HitRecord res = w.res;
    /* The loop's ONE exit stands at its end, on scalar registers: the budget is used up, or no lane has anything left (one minimum, one compare).  The
     * callers enter with a budget of at least one trip and a live lane (entered with none, the first trip finds no lane for either body and leaves). */
    uint32_t left = (uint32_t)budget;
    uint32_t n_leaf = (uint32_t)__popcll(rpt_ballot(SceneViewLds::is_leaf(cur))), n_inner = (uint32_t)__popcll(rpt_ballot(SceneViewLds::is_inner(cur)));
    asm("" : "+s"(n_leaf), "+s"(n_inner));                             /* (scalar registers: see lds_walk_run) */
    uint32_t go;
    do {
        if ((n_leaf << VOTE) > n_inner) {
            if (SceneViewLds::is_leaf(cur)) {
                if constexpr (ONE_TRI) {
                    const uint32_t ti = cur & 511u;
                    const float4 *rec = view.tri_base() + 3u * ti;
                    float t, det;
                    const bool ok = moller_trumbore_flat(xyz4(rec[1]), xyz4(rec[2]), xyz4(rec[0]), ro, rd, t, det);
                    uint32_t next = cur >= LDS_DESC_LEAF_MANY ? cur - LDS_LEAF_REST : LDS_DESC_POP;      /* the rest of the leaf, or the leaf is done */
                    if (ok && t > 0.001f && (SEGMENT ? t < max_t : (t < res.t && (!ANY_HIT || t <= max_t)))) {
                        asm volatile("" ::: "memory");                 /* (a real branch, as in walk_run) */
                        res.t = t;
                        res.tri = ti | (rptm::f2u(det) & 0x80000000u);
                        if (ANY_HIT || (MIXED && stop_first != 0u)) next = LDS_DESC_DEAD;
                    }
                    cur = next;
                } else {
                    bool accepted = false;
                    const uint32_t first = cur & 511u;
                    uint32_t ti = first;
                    const uint32_t end = first + ((cur >> 9) & 63u);       /* (a leaf holds at least one triangle: a count of 0 is an inner node) */
                    const float4 *rec = view.tri_base() + 3u * first;
                    do {
                        float t, det;
                        const bool ok = moller_trumbore_flat(xyz4(rec[1]), xyz4(rec[2]), xyz4(rec[0]), ro, rd, t, det);
                        if (ok && t > 0.001f && (SEGMENT ? t < max_t : (t < res.t && (!ANY_HIT || t <= max_t)))) {
                            asm volatile("" ::: "memory");                 /* (a real branch, as in walk_run) */
                            res.t = t;
                            res.tri = ti | (rptm::f2u(det) & 0x80000000u);
                            if (ANY_HIT || (MIXED && stop_first != 0u)) { accepted = true; break; }
                        }
                        ++ti;
                        rec += 3;
                    } while (ti != end);
                    cur = ((ANY_HIT || MIXED) && accepted) ? LDS_DESC_DEAD : LDS_DESC_POP;
                }
            }
        }
        if ((n_leaf << VOTE) <= n_inner) {                             /* (a branch of its own: as the `else` of the one above, the two are joined through a mask) */
            if (SceneViewLds::is_inner(cur)) {
                const float4 X = lds_planes(px, cur), Y = lds_planes(py, cur), Z = lds_planes(pz, cur);
                const uint32_t d = lds_at<uint32_t>(descs, cur);
                float tl, tr;
                const bool hit_l = slab_pair_lds<true>(X.x, Y.x, Z.x, X.z, Y.z, Z.z, ro_slab, rd, ird, SEGMENT ? max_t : res.t, tl);
                const bool hit_r = slab_pair_lds<true>(X.y, Y.y, Z.y, X.w, Y.w, Z.w, ro_slab, rd, ird, SEGMENT ? max_t : res.t, tr);
                const bool swap = FIXED ? (hit_r && !hit_l)
                                : MIXED ? (hit_r && (!hit_l || tl > tr + order_bias))
                                        : (hit_r && (!hit_l || tl > tr));     /* strict: ties keep left first */
                const uint32_t nf = __builtin_amdgcn_alignbit(d, d, swap ? 16u : 0u);    /* near | far << 16 */
                if (hit_l && hit_r && top < limit) {
                    lds_stack_store(top, nf >> 16);
                    top += LDS_STACK_STRIDE;
                }
                cur = (hit_l || hit_r) ? (nf & 0xffffu) : LDS_DESC_POP;
            }
        }
        if (cur == LDS_DESC_POP) {
            top -= LDS_STACK_STRIDE;
            cur = lds_stack_load(top);
        }
        --left;
        n_leaf = (uint32_t)__popcll(rpt_ballot(SceneViewLds::is_leaf(cur)));
        n_inner = (uint32_t)__popcll(rpt_ballot(SceneViewLds::is_inner(cur)));
        asm("" : "+s"(n_leaf), "+s"(n_inner));
        go = n_leaf + n_inner;
        go = go < left ? go : left;
    } while (go != 0u);
    w.cur = cur;
    w.sp = (int)(top - bottom);
    w.res = res;
}

/* One ray walked to its end: over the LDS image by lds_walk_run (FAST there is SIGNED), over the other views by walk_run. */
template <int STACK, bool ANY_HIT, bool FAST, bool FIXED = false, bool SEGMENT = false, typename View, typename StackRef>
__device__ __forceinline__ HitRecord traverse_loop(const View &view, F3 ro, F3 rd, F3 ird, float max_t, StackRef &stack) {
    Walk<View> w;
    walk_begin(view, w);
    if constexpr (std::is_same<View, SceneViewLds>::value) lds_walk_run<STACK, ANY_HIT, FAST, FIXED, false, SEGMENT>(view, w, ro, rd, ird, max_t, stack, 0x7fffffff);
    else walk_run<STACK, ANY_HIT, FAST, FIXED, SEGMENT>(view, w, ro, rd, ird, max_t, stack, 0x7fffffff);
    return w.res;
}

__device__ __forceinline__ bool fastdiv_ray_ok(uint32_t fastdiv_ok, F3 ro, F3 rd) {
    return fastdiv_ok != 0u && rptm::fastdiv_divisor_ok(rd.x) && rptm::fastdiv_divisor_ok(rd.y) && rptm::fastdiv_divisor_ok(rd.z) &&
           rptm::fastdiv_operand_ok(ro.x) && rptm::fastdiv_operand_ok(ro.y) && rptm::fastdiv_operand_ok(ro.z);
}

template <int STACK, bool ANY_HIT, bool SEGMENT = false, typename View, typename StackT>
__device__ __forceinline__ HitRecord traverse_one(const View &view, uint32_t fastdiv_ok, F3 ro, F3 rd, float max_t, StackT *stack) {
    if (fastdiv_ray_ok(fastdiv_ok, ro, rd)) {
        F3 ird = f3(rptm::rcp_rn_window(rd.x), rptm::rcp_rn_window(rd.y), rptm::rcp_rn_window(rd.z));
        return traverse_loop<STACK, ANY_HIT, true, false, SEGMENT>(view, ro, rd, ird, max_t, stack);
    }
    return traverse_loop<STACK, ANY_HIT, false, false, SEGMENT>(view, ro, rd, rd, max_t, stack);
}

#endif /* RPT_K_WALK_H */
