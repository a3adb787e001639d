/*
 * k_traverse_shadow_kernels.h — the kernels that walk shadow rays (and the one-ray-per-lane test hook), written ONCE and compiled TWICE: k_traverse.h
 * includes this file with
 *     RPT_SHADOW_KERNEL(name) = name,        RPT_SHADOW_KERNEL_SEGMENT = false   the reference's any-hit walk, under the names the kernels always had
 *     RPT_SHADOW_KERNEL(name) = name##_seg,  RPT_SHADOW_KERNEL_SEGMENT = true    the segment-bounded walk of RPT_SHADOW_SEGMENT (k_walk.h
 *                                                                                shadow_segment_bound; rpt.h rpt_set_shadow_mode)
 * so that the exact kernels keep their names, their template argument lists and their code.  (One text, not a body template behind two thin __global__
 * functions: through such a wrapper the compiler schedules the exact kernels differently — one to five instructions more in every one of them — and the
 * default path is not to gain an instruction.)  No include guard, by design.
 */
/* Shadow rays (kernels/src/light_pick.rs:141-148) of a scene the streamed walks cannot take, one ray per lane from global
 * memory: any-hit over the positions of the
 * shadow queue (k_common.h: sharded, dense up to the shards' tails); if unoccluded the pre-weighted NEE contribution is added to the
 * path's radiance (lib.rs:164).  A path that ended at this bounce (bit 31 of
 * the tag) is finished here: accumulated and, if samples remain, regenerated
 * in place (its slot becomes HIT_PENDING again). */
template <int STACK, int THREADS>
__global__ __launch_bounds__(THREADS) void RPT_SHADOW_KERNEL(k_traverse_shadow)(DevScene sc, DevState st, DevQueues q, DevConfig cfg, DevStats *stats) {
    constexpr bool SEGMENT = RPT_SHADOW_KERNEL_SEGMENT;
    __shared__ uint32_t lds_stack[THREADS / RPT_WAVE][STACK][RPT_WAVE];
    if (q.count[Q_DRAINED] != 0u) return;                     /* surplus launch (grid-uniform) */
    uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    uint32_t positions, n;
    q_extent(q.shadow_cnt, positions, n);
    if (i == 0u && n) atomicAdd(&stats->shadow_rays, (unsigned long long)n);
    if (blockIdx.x * THREADS >= positions) return;             /* block-uniform */
    const SceneViewGlobal view{{sc.tri_isect}, sc.nodes};
    if (i >= positions || !q_filled(q.shadow_cnt, i)) return;
    float4 o = q.sh_o[i], d = q.sh_d[i];
    uint32_t tag = __float_as_uint(d.w);
    uint32_t *stack = &lds_stack[threadIdx.x / RPT_WAVE][0][threadIdx.x % RPT_WAVE];
    HitRecord h = traverse_one<STACK, true, SEGMENT>(view, sc.fastdiv_ok, f3(o.x, o.y, o.z), f3(d.x, d.y, d.z), SEGMENT ? shadow_segment_bound(o.w) : o.w, stack);
    shadow_resolve(st, q, cfg, i, tag, h.tri == HIT_MISS);
}

/* Shadow rays of an LDS-resident scene, streamed like the extension rays above (persistent workgroups, spans of the dense
 * shadow queue from a launch-wide counter, refill of finished lanes).  The reference's any-hit walk is not pruned by max_t (it
 * prunes boxes against result.t = 1e6 until something is accepted, intersection.rs:212-213, and box-t / triangle-t
 * round differently: pruning is the opt-in SEGMENT twin, not the exact walk), so an unoccluded ray crosses every box along its
 * line while an occluded one may stop after two visits: lane utilisation of the one-ray-per-lane kernel was 40 % (profiles/r02base_darkcornell_mis_pmc_sq.txt).
 * Lanes only record "occluded" in the unused .w of the entry's contribution record; k_shadow_resolve then adds the NEE
 * terms in one dense pass (all lanes busy, none of the walk's registers live). */
template <int STACK, int THREADS, bool FIXED /* fixed left-first order over the flipped image (shadow_order.h) */>
__attribute__((amdgpu_num_sgpr(RPT_LDS_WALK_SGPRS)))
__global__ __launch_bounds__(THREADS) void RPT_SHADOW_KERNEL(k_traverse_shadow_stream)(DevScene sc, DevState st, DevQueues q, DevStats *stats, uint32_t SPAN) {
    constexpr bool SEGMENT = RPT_SHADOW_KERNEL_SEGMENT;
    constexpr uint32_t NW = THREADS / RPT_WAVE;
    __shared__ uint16_t lds_stack[NW][STACK][RPT_WAVE];
    __shared__ WgPool pool;
    float4 *lds_scene = rpt_lds_dyn;
    if (q.count[Q_DRAINED] != 0u) return;                      /* surplus launch (grid-uniform) */
    uint32_t n, n_entries;                                     /* n: queue positions to hand out */
    q_extent(q.shadow_cnt, n, n_entries);
    uint32_t *global_next = &q.count[Q_SPOOL];                 /* zeroed by the shade stage of this iteration */
    if (blockIdx.x == 0u && threadIdx.x == 0u && n_entries) atomicAdd(&stats->shadow_rays, (unsigned long long)n_entries);
    const uint32_t lane = __lane_id(), wave = threadIdx.x / RPT_WAVE;
    if (threadIdx.x == 0u) {
        const uint32_t g = n ? atomicAdd(global_next, SPAN) : 0u;
        pool.word = wg_pool_span(g, SPAN, n);
        pool.lock = 0u;
    }
    __syncthreads();
    if ((uint32_t)(pool.word >> 32) == 0u) return;             /* block-uniform: nothing (left) to trace */
    const SceneViewLds view = stage_scene_lds<THREADS>(sc, lds_scene, FIXED);
    uint16_t *stack = &lds_stack[wave][0][lane];
    lds_stream_stack_begin(stack);                             /* entry 0 of the lane's column: the sentinel an empty stack pops (k_walk.h lds_stream_walk_run) */
    F3 ro = f3(0, 0, 0), rd = f3(1, 1, 1), ird = f3(1, 1, 1);
    float max_t = 0.0f;
    LdsWalk w;
    walk_begin(view, w);
    w.cur = SceneViewLds::dead();
    uint32_t entry = 0u;
    bool have = false;
    bool pool_open = true;                                     /* wave-uniform */
    for (;;) {
        const unsigned long long idle_m = rpt_ballot(walk_dead(w));
        const uint32_t n_idle = (uint32_t)__popcll(idle_m);
        if (pool_open && n_idle >= (uint32_t)RPT_STREAM_REFILL) {
            uint32_t base = 0u, got = 0u;
            bool finished = false;
            if (lane == 0u) base = wg_pool_take(&pool, global_next, n, SPAN, n_idle, got, finished);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            got = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
            pool_open = __builtin_amdgcn_readfirstlane((int)finished) == 0;
            if (walk_dead(w)) {
                if (have) {
                    q.sh_c[entry].w = w.res.tri == HIT_MISS ? 0.0f : 1.0f;
                    have = false;
                }
                const uint32_t rank = rpt_lane_rank(idle_m);
                if (rank < got && q_filled(q.shadow_cnt, base + rank)) {   /* (a position in the tail of a shard may be empty) */
                    entry = base + rank;
                    const float4 o = q.sh_o[entry], d = q.sh_d[entry];
                    ro = f3(o.x, o.y, o.z); rd = f3(d.x, d.y, d.z);
                    max_t = SEGMENT ? shadow_segment_bound(o.w) : o.w;
                    have = true;
                    if (fastdiv_ray_ok(sc.fastdiv_ok, ro, rd)) {
                        ird = f3(rptm::rcp_rn_window(rd.x), rptm::rcp_rn_window(rd.y), rptm::rcp_rn_window(rd.z));
                        walk_begin(view, w);
                    } else {
                        uint16_t *rest = lds_stream_stack_rest(stack);
                        w.res = traverse_loop<STACK - 1, true, false, FIXED, SEGMENT>(view, ro, rd, rd, max_t, rest);   /* alone; recorded at the next refill */
                    }
                }
            }
            if (got != 0u || !pool_open) continue;
            if (idle_m == ~0ull) { __builtin_amdgcn_s_sleep(8); continue; }   /* another wave is fetching the next span */
        }
        if (idle_m == ~0ull) {
            if (!pool_open) break;                             /* nothing in flight and nothing left to hand out */
            continue;
        }
        lds_stream_walk_run<STACK, true, FIXED, false, false, SEGMENT>(view, w, ro, rd, ird, max_t, stack, pool_open ? RPT_STREAM_TRIPS : 0x7fffffff);
    }
    if (have) q.sh_c[entry].w = w.res.tri == HIT_MISS ? 0.0f : 1.0f;
}

/* Shadow rays, streamed: the queue is dense already (up to the tails of its shards); a wave owns SPAN consecutive positions and refills lanes whose
 * any-hit walk has ended (found an occluder after two visits, or crossed the whole scene without one).  Lanes only note
 * "occluded" per entry in LDS while walking; the NEE terms are added afterwards in one dense pass over the span (all
 * lanes busy, and the registers of the walk are dead by then: 61 instead of 91 VGPRs). */
template <int STACK, int WIDTH, bool COOP, bool FIXED /* fixed left-first order over the flipped pair array (shadow_order.h) */>
__attribute__((amdgpu_waves_per_eu(gstream_waves(STACK, WIDTH, COOP), 8)))
 __global__ __launch_bounds__(RPT_WAVE) void RPT_SHADOW_KERNEL(k_traverse_shadow_gstream)(DevScene sc, DevState st, DevQueues q, DevConfig cfg, DevStats *stats,
                                                                      uint32_t SPAN) {
    constexpr bool SEGMENT = RPT_SHADOW_KERNEL_SEGMENT;
    __shared__ WaveStack<STACK, WIDTH> lds_stack;
    __shared__ uint8_t occluded[RPT_WAVE * RPT_GSTREAM_RAYS];
    if (q.count[Q_DRAINED] != 0u) return;                      /* surplus launch (grid-uniform) */
    const uint32_t lane = threadIdx.x;
    uint32_t n, n_entries;                                     /* n: queue positions of the launch */
    q_extent(q.shadow_cnt, n, n_entries);
    if (blockIdx.x == 0u && lane == 0u && n_entries) atomicAdd(&stats->shadow_rays, (unsigned long long)n_entries);
    const uint32_t begin = blockIdx.x * SPAN;
    if (begin >= n) return;
    const uint32_t end = begin + SPAN < n ? begin + SPAN : n;
    {
        typedef SceneViewPairsT<COOP> View;
        const View view = FIXED ? View{{sc.tri_isect}, sc.gpairs_shadow, sc.glinks_shadow} : View{{sc.tri_isect}, sc.gpairs, sc.glinks};
        auto stack = lds_stack.column(lane);
        F3 ro = f3(0, 0, 0), rd = f3(1, 1, 1), ird = f3(1, 1, 1);
        float max_t = 0.0f;
        Walk<View> w;
        walk_begin(view, w);
        w.cur = View::dead();
        uint32_t entry = 0u, next = begin;                     /* next: wave-uniform */
        bool have = false;
        for (;;) {
            const unsigned long long idle_m = rpt_ballot(walk_dead(w));
            const uint32_t n_idle = (uint32_t)__popcll(idle_m);
            const bool more = next < end;                      /* wave-uniform */
            if ((more && n_idle >= (uint32_t)RPT_GSTREAM_REFILL) || idle_m == ~0ull) {
                if (walk_dead(w)) {
                    if (have) {
                        occluded[entry - begin] = w.res.tri == HIT_MISS ? (uint8_t)0 : (uint8_t)1;
                        have = false;
                    }
                    const uint32_t at = next + rpt_lane_rank(idle_m);
                    if (at < end && q_filled(q.shadow_cnt, at)) {
                        const float4 o = q.sh_o[at], d = q.sh_d[at];
                        ro = f3(o.x, o.y, o.z); rd = f3(d.x, d.y, d.z);
                        max_t = SEGMENT ? shadow_segment_bound(o.w) : o.w;
                        entry = at;
                        have = true;
                        if (fastdiv_ray_ok(sc.fastdiv_ok, ro, rd)) {
                            ird = f3(rptm::rcp_rn_window(rd.x), rptm::rcp_rn_window(rd.y), rptm::rcp_rn_window(rd.z));
                            walk_begin(view, w);
                        } else {
                            w.res = traverse_loop<STACK, true, false, FIXED, SEGMENT>(view, ro, rd, rd, max_t, stack);   /* alone; noted at the next refill */
                        }
                    }
                }
                if (!more) break;
                next += n_idle;
                continue;
            }
            walk_run<STACK, true, true, FIXED, SEGMENT>(view, w, ro, rd, ird, max_t, stack, more ? RPT_GSTREAM_TRIPS : 0x7fffffff);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t base = begin; base < end; base += RPT_WAVE) {
        const uint32_t e = base + lane;
        if (e < end && q_filled(q.shadow_cnt, e)) shadow_resolve(st, q, cfg, e, __float_as_uint(q.sh_d[e].w), occluded[e - begin] == 0u);
    }
}

/* Test hook: plain ray arrays in, hit arrays out (rpt_debug_trace_rays; k_trace_debug_seg: any_hit = 2, the segment-bounded any-hit walk). */
template <int STACK, bool ANY_HIT, bool LDS_SCENE, int THREADS>
__global__ __launch_bounds__(THREADS) void RPT_SHADOW_KERNEL(k_trace_debug)(DevScene sc, uint32_t n, const float *origins, const float *dirs,
                                                         const float *max_t, float *out_t, uint32_t *out_tri, uint32_t *out_flags) {
    constexpr bool SEGMENT = RPT_SHADOW_KERNEL_SEGMENT && ANY_HIT;
    /* LDS-resident scenes walk 16-bit descriptors: 16-bit stack entries (32 KB per 1024-thread workgroup, which with a
     * <= 32 KB scene image is the 64 KB a workgroup may hold: 2 workgroups = 32 waves per CU) */
    typedef typename StackElem<LDS_SCENE>::type StackT;
    __shared__ StackT lds_stack[THREADS / RPT_WAVE][STACK][RPT_WAVE];
    float4 *lds_scene = rpt_lds_dyn;
    uint32_t i = blockIdx.x * THREADS + threadIdx.x;
    const auto view = stage_scene<LDS_SCENE, THREADS>(sc, lds_scene);
    if (i >= n) return;
    F3 ro = f3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]);
    F3 rd = f3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]);
    StackT *stack = &lds_stack[threadIdx.x / RPT_WAVE][0][threadIdx.x % RPT_WAVE];
    HitRecord h = traverse_one<STACK, ANY_HIT, SEGMENT>(view, sc.fastdiv_ok, ro, rd, ANY_HIT ? (SEGMENT ? shadow_segment_bound(max_t[i]) : max_t[i]) : 0.0f, stack);
    out_t[i] = h.t;
    out_tri[i] = (h.tri == HIT_MISS) ? 0u : (h.tri & 0x7fffffffu);
    out_flags[i] = (h.tri == HIT_MISS) ? 0u : (1u | ((h.tri >> 31) << 1));
}
