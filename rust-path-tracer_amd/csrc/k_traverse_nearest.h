/*
 * k_traverse_nearest.h — the kernels that walk EXTENSION rays (nearest hit): one ray per lane from global memory, streamed over the LDS image, streamed
 * through global memory.
 */
#ifndef RPT_K_TRAVERSE_NEAREST_H
#define RPT_K_TRAVERSE_NEAREST_H

#include "k_path.h"
#include "k_walk_stream.h"

/* Extension rays of a scene the streamed walks cannot take (a node pool that is not pair-shaped), one ray per lane from
 * global memory.  Thread i owns slot i; it traces the slot's ray if one is
 * pending (HIT_PENDING) and writes the hit record into hit[slot].  A wave that
 * found work raises this iteration's alive flag (plain store, every writer
 * stores the same value), which the shade stage reports to the host. */
template <int STACK, int THREADS>
__global__ __launch_bounds__(THREADS) void k_traverse_nearest(DevScene sc, DevState st, DevQueues q, uint32_t iteration) {
    __shared__ uint32_t lds_stack[THREADS / RPT_WAVE][STACK][RPT_WAVE];
    if (q.count[Q_DRAINED] != 0u) return;                      /* surplus launch (grid-uniform) */
    const uint32_t slot = blockIdx.x * THREADS + threadIdx.x;
    if (slot == 0u) {
        iteration_bookkeeping(q, iteration);
    }
    bool pending = false;
    if (slot < st.n_slots) pending = __float_as_uint(st.hit[slot].y) == HIT_PENDING;
    const SceneViewGlobal view{{sc.tri_isect}, sc.nodes};
    unsigned long long active = rpt_ballot(pending);
    if (active == 0ull) return;
    if (__lane_id() == (uint32_t)__ffsll((long long)active) - 1u) {
        raise_flag(&q.count[Q_ALIVE0 + (iteration & 1u) * Q_LINE]);
        /* ray accounting: sharded, non-returning atomics (nobody waits for them) */
        atomicAdd(&q.ray_shards[(blockIdx.x % RPT_STAT_SHARDS) * RPT_STAT_STRIDE], (unsigned long long)__popcll(active));
    }
    if (!pending) return;
    float4 ra = st.ray_a[slot];
    float2 rb = st.ray_b[slot];
    F3 ro = f3(ra.x, ra.y, ra.z), rd = f3(ra.w, rb.x, rb.y);
    uint32_t *stack = &lds_stack[threadIdx.x / RPT_WAVE][0][threadIdx.x % RPT_WAVE];
    HitRecord h = traverse_one<STACK, false>(view, sc.fastdiv_ok, ro, rd, 0.0f, stack);
    store_hit(st, slot, h);
}

/* Extension rays of an LDS-resident scene, STREAMED: a workgroup takes spans of consecutive slots (between 1 and 8 per
 * lane, rpt_traverse.hip lds_stream_span) and deals them to the idle lanes of its waves on demand.
 * The traversal is VALU-issue bound and after the first bounce the rays of a wave need very different numbers of
 * trips (DarkCornell bounce 2: median 25, p90 34, max 68 node visits), so a one-ray-per-lane wave spends most of its
 * trips with a minority of lanes alive (lane utilisation 40 %).  Here, every RPT_STREAM_TRIPS trips the wave looks at
 * its idle lanes; when at least RPT_STREAM_REFILL are idle they write their hit records and take the next slots from the
 * workgroup's pool (below).  The walk itself (lds_stream_walk_run) runs with a trip budget: no per-lane bookkeeping inside
 * the hot loop.  Per ray nothing changes — same tests in the same order — so hit records are the reference's bit for
 * bit, and slots stay identity mapped (a slot's ray is traced by SOME lane of the wave that owns its range). */
/* LAST: the launch that traces the last extension ray of every path of a batch of known length WITHOUT NEE (the host's choice, rpt_hip.hip launch_iteration:
 * the same condition as the shade stage's last_iteration).  At that bounce the reference reads three things off the walk's result (kernels/src/lib.rs:62-109):
 * a miss adds the sky; a hit on the front of a triangle whose material emits adds its emission; any other hit adds nothing and ends the sample.  A ray that
 * passes the Moller-Trumbore test of NO emissive triangle (sc.last_emit_tri, at most RPT_LAST_EMIT_MAX of them, tested when the lane takes the ray) cannot
 * end on one, so "hit or miss" is all its walk has to say: it stops at its first accepted triangle (lds_stream_walk_run MIXED) — in a closed scene about half of
 * the node visits of the bounce (tools/last_bounce_sim.py).  Its hit record names THAT triangle: not the nearest one, but like the nearest one not an
 * emitter, which is all the shade stage's last iteration looks at.  A ray that does pass such a test runs the reference's walk to its end. */
/* FIRST: the launch of a render call's first iteration, where every ray is a camera ray and leaves cfg.cam_position (k_path.h camera_ray; lib.rs:36-60):
 * the workgroup stages the plane records with that origin subtracted (lds_stream_walk_run PRESUB) — twelve of the ~ 98 instructions of a node-pair step. */
#define RPT_NEAREST_PLAIN 0
#define RPT_NEAREST_LAST 1
#define RPT_NEAREST_FIRST 2
template <int STACK, int THREADS, int MODE = RPT_NEAREST_PLAIN>
__attribute__((amdgpu_num_sgpr(RPT_LDS_WALK_SGPRS)))
__global__ __launch_bounds__(THREADS) void k_traverse_nearest_stream(DevScene sc, DevState st, DevQueues q, uint32_t iteration,
                                                                       uint32_t SPAN /* slots a workgroup fetches at a time */,
                                                                       float cam_x, float cam_y, float cam_z /* FIRST: the origin of every ray of the launch */,
                                                                       DevConfig cfg, uint32_t gen_samples /* FIRST: the call's sample count when the walk starts the first
                                                                       paths itself (wave-uniform; 0: the slots were prepared by k_generate_first, HIT_PENDING) */,
                                                                       DevStats *stats) {
    constexpr bool LAST = MODE == RPT_NEAREST_LAST, FIRST = MODE == RPT_NEAREST_FIRST;
    constexpr uint32_t NW = THREADS / RPT_WAVE;
    __shared__ uint16_t lds_stack[NW][STACK][RPT_WAVE];
    __shared__ WgPool pool;
    float4 *lds_scene = rpt_lds_dyn;
    if (q.count[Q_DRAINED] != 0u) return;                      /* surplus launch (grid-uniform) */
    uint32_t *global_next = &q.count[Q_POOL0 + (iteration & 1u) * Q_LINE];
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        /* per-iteration bookkeeping, as in k_traverse_nearest (+ the other parity's slot counter, unused in this launch) */
        iteration_bookkeeping(q, iteration);
        q.count[Q_POOL0 + ((iteration + 1u) & 1u) * Q_LINE] = 0u;
    }
    const uint32_t lane = __lane_id(), wave = threadIdx.x / RPT_WAVE;
    if (threadIdx.x == 0u) {
        const uint32_t g = atomicAdd(global_next, SPAN);
        pool.word = wg_pool_span(g, SPAN, st.n_slots);
        pool.lock = 0u;
    }
    __syncthreads();
    if ((uint32_t)(pool.word >> 32) == 0u) return;             /* block-uniform: a late workgroup, nothing left */
    /* LAST: behind the image, the pair records (planes + child descriptors) of the flipped copy the hit-or-miss lanes walk in fixed order, when the
     * scene has one and the host found room for it (sc.last_flip_vecs float4; 0: those lanes walk the primary image near child first) */
    if (LAST)
        for (uint32_t k = threadIdx.x; k < sc.last_flip_vecs; k += THREADS) lds_scene[sc.lds_vecs + k] = sc.lds_image_last[k];
    if (FIRST) {
        const uint32_t P2 = 2u * sc.lds_pairs;                 /* image layout (rpt_scene.hip build_lds_image): 2 P plane records per axis, x | y | z */
        for (uint32_t k = threadIdx.x; k < 3u * P2; k += THREADS) {
            const float4 v = sc.lds_image[k];
            const float o = k < P2 ? cam_x : (k < 2u * P2 ? cam_y : cam_z);
            lds_scene[k] = make_float4(v.x - o, v.y - o, v.z - o, v.w - o);
        }
        for (uint32_t k = 3u * P2 + threadIdx.x; k < sc.lds_vecs; k += THREADS) lds_scene[k] = sc.lds_image[k];
        __syncthreads();
    }
    const SceneViewLds view = FIRST ? SceneViewLds{lds_scene, sc.lds_pairs, sc.n_triangles, sc.lds_root} : stage_scene_lds<THREADS>(sc, lds_scene);
    const float4 *img_lane = view.img;                         /* (per lane, LAST only) */
    uint32_t stop_first = 0u;
    float order_bias = 0.0f;
    uint16_t *stack = &lds_stack[wave][0][lane];
    lds_stream_stack_begin(stack);                             /* entry 0 of the lane's column: the sentinel an empty stack pops (k_walk.h lds_stream_walk_run) */
    F3 ro = f3(0, 0, 0), rd = f3(1, 1, 1), ird = f3(1, 1, 1);
    LdsWalk w;
    walk_begin(view, w);
    w.cur = SceneViewLds::dead();
    uint32_t slot = 0u;
    bool have = false;                                         /* this lane holds a ray whose result is not written yet */
    bool pool_open = true;                                     /* wave-uniform: the launch may still have slots */
    uint32_t traced = 0u;                                      /* wave-uniform */
    /* LAST with several slots per pixel: the walk ENDS its paths — no shade launch follows it (rpt_hip.hip launch_iteration).  Where a lane writes its result it does
     * what the shade stage's last iteration did with it (k_shade.h shade_slot, `last_iteration`):
     *   a hit-or-miss lane that hit: not an emitter, the sample is finished with the zero radiance it has — HIT_DONE_ZERO;
     *   a lane that walked to the end and hit: the front of an emitter adds its emission (lib.rs:86-100) — the radiance record is written, HIT_DONE; any other
     *   hit is HIT_DONE_ZERO;
     *   a miss: the slot goes to the sky queue (last_park below) and waits there as HIT_PARKED for the batch's one k_sky launch.
     * Such a batch keeps no radiance record of a live path (DevQueues::implicit_zero: the launch is LAST only in a batch of known length without NEE, so the
     * flag says "several slots per pixel" here): nothing is read, 0 + the term is written.
     * With one slot per pixel (done_here false) the hit record is written for the shade launch that follows, as in every other launch. */
    const bool done_here = LAST && q.implicit_zero != 0u;
    auto last_finish = [&](uint32_t s, const HitRecord &r, uint32_t stopped) -> bool {      /* true: a miss, to be parked */
        if (!done_here) {
            store_hit(st, s, r);
            return false;
        }
        if (r.tri == HIT_MISS) return true;
        if (stopped == 0u) {
            const uint32_t m = __float_as_uint(sc.tri_shade[4u * (r.tri & 0x7fffffffu) + 2u].w);
            const float4 e4 = sc.textured != 0u ? sc.materials[6u * m] : sc.mat_lite[2u * m];
            if ((e4.x != 0.0f || e4.y != 0.0f || e4.z != 0.0f) && (r.tri >> 31) == 0u) {
                const float4 tf = st.thr[s];
                finish_from_zero(st, s, mask_nan3(f3(tf.x, tf.y, tf.z) * f3(e4.x, e4.y, e4.z)));
                return false;
            }
        }
        set_hit_word(st, s, HIT_DONE_ZERO);
        return false;
    };
    /* The sky queue's reservations, by the whole wave (every lane calls it, converged).  A slot is reserved in the shard the shade stage of this batch uses for
     * it — workgroup b of k_shade pushes into shard b % RPT_Q_SHARDS and owns 1 << q.sky_shard_shift slots (256, packed variant 2 048) — and a slot misses at
     * most once per batch, so a shard never receives more entries than its workgroups own slots: the bound RPT_Q_SLACK was sized for.  One returning atomic per
     * wave and shard: the lanes of a wave took their slots in runs of consecutive ones, so a few shards cover them. */
    auto last_park = [&](bool park, uint32_t s) {
        const uint32_t shard = (s >> q.sky_shard_shift) % RPT_Q_SHARDS;
        unsigned long long todo_m = rpt_ballot(park);
        while (todo_m != 0ull) {                               /* wave-uniform */
            const uint32_t leader = (uint32_t)__ffsll((long long)todo_m) - 1u;
            const uint32_t sh = (uint32_t)__builtin_amdgcn_readlane((int)shard, (int)leader);
            const bool mine = park && shard == sh;
            const unsigned long long same = rpt_ballot(mine);
            uint32_t e = 0u;
            if (lane == leader) e = atomicAdd(&q.sky_cnt[sh * RPT_Q_SHARD_STRIDE], (uint32_t)__popcll(same));
            e = (uint32_t)__builtin_amdgcn_readlane((int)e, (int)leader);
            if (mine) {
                e += rpt_lane_rank(same);
                q.sky[q_position(sh, e)] = s;
                set_hit_word(st, s, HIT_PARKED);
            }
            todo_m &= ~same;
        }
    };
    for (;;) {
        const unsigned long long idle_m = rpt_ballot(walk_dead(w));
        const uint32_t n_idle = (uint32_t)__popcll(idle_m);
        if (pool_open && n_idle >= (uint32_t)RPT_STREAM_REFILL) {
            uint32_t base = 0u, got = 0u;
            bool finished = false;
            if (lane == 0u) base = wg_pool_take(&pool, global_next, st.n_slots, SPAN, n_idle, got, finished);
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            got = (uint32_t)__builtin_amdgcn_readfirstlane((int)got);
            pool_open = __builtin_amdgcn_readfirstlane((int)finished) == 0;
            bool took = false;
            if (LAST) {
                const bool writes = walk_dead(w) && have;
                bool park = false;
                if (writes) {
                    park = last_finish(slot, w.res, stop_first);
                    have = false;
                }
                if (done_here) last_park(park, slot);
            }
            if (walk_dead(w)) {
                if (!LAST && have) {
                    store_hit(st, slot, w.res);
                    have = false;
                }
                const uint32_t rank = rpt_lane_rank(idle_m);
                if (rank < got) {
                    const uint32_t cand = base + rank;
                    const uint32_t word = __float_as_uint(st.hit[cand].y);
                    bool pending;
                    if (FIRST && gen_samples != 0u) {
                        /* the slot's first path of the call begins here: its camera ray is a function of (slot, rng[pixel]) (k_path.h) */
                        pending = begin_first_path(st, cfg, stats, cand, word, gen_samples, ro, rd);
                    } else {
                        pending = word == HIT_PENDING;
                        if (pending) {
                            const float4 ra = st.ray_a[cand];
                            const float2 rb = st.ray_b[cand];
                            ro = f3(ra.x, ra.y, ra.z); rd = f3(ra.w, rb.x, rb.y);
                        }
                    }
                    if (pending) {
                        slot = cand;
                        took = true;
                        if (fastdiv_ray_ok(sc.fastdiv_ok, ro, rd)) {
                            ird = f3(rptm::rcp_rn_window(rd.x), rptm::rcp_rn_window(rd.y), rptm::rcp_rn_window(rd.z));
                            walk_begin(view, w);
                            have = true;
                            if (LAST) {
                                bool may_emit = false;
                                for (uint32_t e = 0; e < sc.last_emit_n; ++e) {
                                    float t_e;
                                    bool bf_e;
                                    may_emit = moller_trumbore_view(view, sc.last_emit_tri[e], ro, rd, t_e, bf_e) || may_emit;
                                }
                                stop_first = may_emit ? 0u : 1u;
                                const bool flipped = !may_emit && sc.last_flip_vecs != 0u;
                                img_lane = flipped ? view.img + sc.lds_vecs : view.img;
                                order_bias = flipped ? __builtin_inff() : 0.0f;
                            }
                        } else {
                            /* outside the exact-division guard (a zero / denormal-small direction component): walked here, alone */
                            LdsWalk alone;
                            walk_begin(view, alone);
                            lds_walk_run<STACK - 1, false, false, false, FIRST>(view, alone, ro, rd, rd, 0.0f, lds_stream_stack_rest(stack), 0x7fffffff);
                            if (LAST) {
                                /* the reference's walk to its end; the lane stays idle and ends the path where it next writes (the next refill, or the tail) */
                                w.res = alone.res;
                                stop_first = 0u;
                                have = true;
                            } else {
                                store_hit(st, cand, alone.res);
                            }
                        }
                    }
                }
            }
            traced += (uint32_t)__popcll(rpt_ballot(took));
            if (got != 0u || !pool_open) continue;             /* slots that were not pending leave lanes idle: look again */
            if (idle_m == ~0ull) { __builtin_amdgcn_s_sleep(8); continue; }   /* another wave is fetching the next span */
        }
        if (idle_m == ~0ull) {
            if (!pool_open) break;                             /* nothing in flight and nothing left to hand out */
            continue;
        }
        if (LAST) lds_stream_walk_run<STACK, false, false, true>(view, w, ro, rd, ird, 0.0f, stack, pool_open ? RPT_STREAM_TRIPS : 0x7fffffff, img_lane, stop_first, order_bias);
        else lds_stream_walk_run<STACK, false, false, false, FIRST, false, FIRST ? 0 : RPT_STREAM_PLAIN_VOTE, !FIRST && RPT_STREAM_PLAIN_ONE_TRI>(view, w, ro, rd, ird, 0.0f, stack, pool_open ? RPT_STREAM_TRIPS : 0x7fffffff);
    }
    if (LAST) {
        bool park = false;
        if (have) park = last_finish(slot, w.res, stop_first);
        if (done_here) last_park(park, slot);
    } else if (have) {
        store_hit(st, slot, w.res);
    }
    /* ray accounting + the alive flag, once per wave */
    if (lane == 0u && traced != 0u) {
        raise_flag(&q.count[Q_ALIVE0 + (iteration & 1u) * Q_LINE]);
        atomicAdd(&q.ray_shards[(blockIdx.x % RPT_STAT_SHARDS) * RPT_STAT_STRIDE], (unsigned long long)traced);
    }
}

template <int STACK, int WIDTH /* bits of a stack entry: 16, 21, 24, 32 */, bool COOP /* the scene has leaves of more than RPT_COOP_LEAF_MIN triangles */>
__attribute__((amdgpu_waves_per_eu(gstream_waves(STACK, WIDTH, COOP), 8)))
 __global__ __launch_bounds__(RPT_WAVE) void k_traverse_nearest_gstream(DevScene sc, DevState st, DevQueues q, uint32_t iteration,
                                                                       uint32_t SPAN /* slots per wave, <= 64 * gstream_rays_nearest(STACK, WIDTH) */) {
    __shared__ WaveStack<STACK, WIDTH> lds_stack;
    __shared__ uint16_t pend[RPT_WAVE * gstream_rays_nearest(STACK, WIDTH)];
    if (q.count[Q_DRAINED] != 0u) return;                      /* surplus launch (grid-uniform) */
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x == 0u && lane == 0u) {
        /* per-iteration bookkeeping, as in k_traverse_nearest */
        iteration_bookkeeping(q, iteration);
    }
    const uint32_t span_begin = blockIdx.x * SPAN;
    if (span_begin >= st.n_slots) return;
    const uint32_t span_end = span_begin + SPAN < st.n_slots ? span_begin + SPAN : st.n_slots;
    uint32_t count = 0u;                                       /* wave-uniform */
    /* the pending slots of the span, in slot order */
    for (uint32_t base = span_begin; base < span_end; base += RPT_WAVE) {
        const uint32_t s = base + lane;
        const bool p = s < span_end && __float_as_uint(st.hit[s].y) == HIT_PENDING;
        const unsigned long long m = rpt_ballot(p);
        if (p) pend[count + rpt_lane_rank(m)] = (uint16_t)(s - span_begin);
        count += (uint32_t)__popcll(m);
    }
    if (count == 0u) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0u) {
        raise_flag(&q.count[Q_ALIVE0 + (iteration & 1u) * Q_LINE]);
        atomicAdd(&q.ray_shards[(blockIdx.x % RPT_STAT_SHARDS) * RPT_STAT_STRIDE], (unsigned long long)count);
    }
    typedef SceneViewPairsT<COOP> View;
    const View view{{sc.tri_isect}, sc.gpairs, sc.glinks};
    auto stack = lds_stack.column(lane);
    F3 ro = f3(0, 0, 0), rd = f3(1, 1, 1), ird = f3(1, 1, 1);
    Walk<View> w;
    walk_begin(view, w);
    w.cur = View::dead();
    uint32_t slot = 0u, next = 0u;                             /* next: wave-uniform position in the list */
    bool have = false;                                         /* this lane holds a ray whose result is not written yet */
    /* The first iteration of a batch walks CAMERA rays: the 64 slots a wave deals together are one 8 x 8 pixel block at one sample index, their
     * rays stand on the same node step after step (k_walk.h children_uniform: the scalar-cache path) and end within a few steps of each other.
     * A refill would put rays at the root beside rays deep in the tree and end that: there the wave takes its next 64 slots only when all are done. */
    const uint32_t refill_at = iteration == 0u ? (uint32_t)RPT_GSTREAM_REFILL_FIRST : (uint32_t)RPT_GSTREAM_REFILL;
    for (;;) {
        const unsigned long long idle_m = rpt_ballot(walk_dead(w));
        const uint32_t n_idle = (uint32_t)__popcll(idle_m);
        const bool more = next < count;                        /* wave-uniform */
        if ((more && n_idle >= refill_at) || idle_m == ~0ull) {
            if (walk_dead(w)) {
                if (have) {
                    store_hit(st, slot, w.res);
                    have = false;
                }
                const uint32_t at = next + rpt_lane_rank(idle_m);
                if (at < count) {
                    slot = span_begin + pend[at];
                    const float4 ra = st.ray_a[slot];
                    const float2 rb = st.ray_b[slot];
                    ro = f3(ra.x, ra.y, ra.z); rd = f3(ra.w, rb.x, rb.y);
                    have = true;
                    if (fastdiv_ray_ok(sc.fastdiv_ok, ro, rd)) {
                        ird = f3(rptm::rcp_rn_window(rd.x), rptm::rcp_rn_window(rd.y), rptm::rcp_rn_window(rd.z));
                        walk_begin(view, w);
                    } else {
                        /* outside the exact-division guard (a zero / denormal-small direction component): walked here, alone;
                         * the lane stays idle and writes the result at its next refill */
                        w.res = traverse_loop<STACK, false, false>(view, ro, rd, rd, 0.0f, stack);
                    }
                }
            }
            if (!more) break;                                  /* everything handed out, walked and written */
            next += n_idle;
            continue;
        }
        walk_run<STACK, false, true>(view, w, ro, rd, ird, 0.0f, stack, more ? RPT_GSTREAM_TRIPS : 0x7fffffff);
    }
}

#endif /* RPT_K_TRAVERSE_NEAREST_H */
