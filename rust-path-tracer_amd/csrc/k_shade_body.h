/*
 * k_shade_body.h — the text of the surface stage's kernel (k_shade.h describes it), compiled once per kernel that shares it, as k_complete_body.h is:
 * k_shade (k_shade.h), k_shade_models (rpt_models.hip) for a context whose materials carry models (rpt_set_material_models), and k_shade_volumes
 * (rpt_volumes.hip) for one whose Glass materials absorb (rpt_set_material_volumes), and k_shade_punctual (rpt_punctual.hip) for one that has punctual lights
 * (rpt_set_punctual_lights).  The includer defines
 *   RPT_SHADE_KERNEL          the kernel's name
 *   RPT_SHADE_MODELS          shade_slot's MODELS: false / true
 *   RPT_SHADE_MODELS_ARG(...) its argument in the models build — the records, a kernel argument of their own and not a field of DevScene, which every stage
 *                             kernel takes — and nothing in the plain one, so k_shade is compiled from the text it always had
 *   RPT_SHADE_VOLUMES         shade_slot's VOLUMES: false / true (true only with MODELS)
 *   RPT_SHADE_VOLUMES_ARG(...) its argument in the volumes build, the volume records, in the same way
 *   RPT_SHADE_PUNCTUAL        shade_slot's PUNCTUAL: false / true (true only with MODELS and VOLUMES)
 *   RPT_SHADE_PUNCTUAL_ARG(...) its argument in the punctual build, the lights with their count and share (k_punctual.h DevPunctual), in the same way
 *   RPT_SHADE_OCCUPANCY       the waves per SIMD asked of the compiler (k_shade.h RPT_SHADE_WAVES_*), or nothing
 * (A function template over MODELS that both kernels call was tried first: inlined, it did not give k_shade the instruction stream it had.)
 */
template <int NEE, bool TEXTURED, bool COMPACT>
RPT_SHADE_OCCUPANCY
__global__ __launch_bounds__(RPT_BLOCK) void RPT_SHADE_KERNEL(DevScene sc, DevState st, DevQueues q, DevConfig cfg, uint32_t iteration,
                                                              DevStats *stats, uint32_t n_samples /* of this render call */
                                                              RPT_SHADE_MODELS_ARG(, const uint4 *models /* one record per material, or null: every material PBR */)
                                                              RPT_SHADE_VOLUMES_ARG(, const float4 *volumes /* one record per material, or null: no material absorbs */)
                                                              RPT_SHADE_PUNCTUAL_ARG(, DevPunctual pl /* the punctual lights, or n == 0 */)) {
    const bool first_paths = iteration == 0u;                  /* every traversed slot holds the first path of its call (k_path.h) */
    /* a batch of known length: iteration i shades bounce i of every path, so its last iteration is every path's last bounce (not the first one: a first
       path has no radiance record yet) */
    const bool last_iteration = q.known_length != 0u && iteration != 0u && iteration + 1u >= cfg.c.max_bounces;
    __shared__ uint32_t push_scratch[RPT_BLOCK / RPT_WAVE + 1];
    __shared__ uint32_t c_slot[COMPACT ? RPT_BLOCK * RPT_SHADE_ROUNDS : 1];
    __shared__ uint32_t n_elided;                              /* NEE evaluations of this workgroup whose shadow ray was not queued (shade_slot) */
    if (q.count[Q_DRAINED] != 0u) return;                      /* surplus launch (grid-uniform) */
    if (NEE != RPT_NEE_NONE) {
        if (threadIdx.x == 0u) n_elided = 0u;
        __syncthreads();                                       /* before any wave's count_elided (one barrier per workgroup; block-uniform: the returns above are) */
    }
    if (NEE != RPT_NEE_NONE && blockIdx.x == 0u && threadIdx.x == 0u) q.count[Q_SPOOL] = 0u;   /* the shadow stage that follows starts its pool at entry 0 */
    if (COMPACT) {
        const uint32_t base = blockIdx.x * (RPT_BLOCK * RPT_SHADE_ROUNDS);
        if (base >= st.n_slots) return;                        /* block-uniform */
        float2 hws[RPT_SHADE_ROUNDS];
#pragma unroll
        for (int r = 0; r < RPT_SHADE_ROUNDS; ++r) {           /* all looks in flight before the first is used */
            const uint32_t s0 = base + (uint32_t)r * RPT_BLOCK + threadIdx.x;
            hws[r] = s0 < st.n_slots ? st.hit[s0] : make_float2(0.0f, __uint_as_float(HIT_PARKED));
        }
        /* Binned by what the stage will do with the slot (lib.rs:64-79 vs :80-181): HITS fill the list from the front, MISSES from the back, and the
         * hits are padded to whole waves — so no wave holds both.  A miss only parks its slot and queues it for the sky stage (~25 instructions); in
         * slot order it sat beside lanes running the ~1 400-instruction surface body: from the second bounce on 40-80 % of the traversed slots of an
         * open scene are misses, the stage ran at 45 % lanes (profiles/r04_{veachmis,pbrtest}_pmc_sq.txt; tools/shade_bin_sim.py replays it:
         * 26-31 % fewer wave-instructions).  The order inside the list is no part of any result: every entry touches only its own slot. */
        constexpr uint32_t CAP = RPT_BLOCK * RPT_SHADE_ROUNDS;
        uint32_t total_h = 0u, total_m = 0u;                   /* block-uniform */
#pragma unroll
        for (int r = 0; r < RPT_SHADE_ROUNDS; ++r) {
            const uint32_t s0 = base + (uint32_t)r * RPT_BLOCK + threadIdx.x;
            const uint32_t word = __float_as_uint(hws[r].y);
            const bool is_hit = word < HIT_IDLE, is_miss = word == HIT_MISS;
            uint32_t ih, im, nh, nm;
            block_rank2(is_hit, is_miss, push_scratch, ih, im, nh, nm);
            if (is_hit) c_slot[total_h + ih] = s0;
            if (is_miss) c_slot[CAP - 1u - (total_m + im)] = s0;
            total_h += nh; total_m += nm;
        }
        __syncthreads();
        const uint32_t hits_padded = (total_h + RPT_WAVE - 1u) & ~(uint32_t)(RPT_WAVE - 1u);
        const uint32_t total = hits_padded + total_m;
        for (uint32_t first = 0u; first < total; first += RPT_BLOCK) {      /* block-uniform trip count */
            const uint32_t v = first + threadIdx.x;
            const bool a_hit = v < total_h, a_miss = v >= hits_padded && v < total;
            const bool active = a_hit || a_miss;
            const uint32_t slot = a_hit ? c_slot[v] : (a_miss ? c_slot[CAP - 1u - (v - hits_padded)] : 0u);
            const float2 hw = a_hit ? st.hit[slot] : make_float2(0.0f, __uint_as_float(a_miss ? HIT_MISS : HIT_PARKED));
            bool to_sky = false, emit_shadow = false, elided = false;
            float4 sh_o = make_float4(0, 0, 0, 0), sh_d = sh_o, sh_c = sh_o;
            shade_slot<NEE, TEXTURED, true, RPT_SHADE_MODELS, RPT_SHADE_VOLUMES, RPT_SHADE_PUNCTUAL>(sc, st, q, cfg, stats, slot, hw, active, to_sky, emit_shadow, sh_o, sh_d, sh_c, first_paths, n_samples, elided, last_iteration RPT_SHADE_MODELS_ARG(, models) RPT_SHADE_VOLUMES_ARG(, volumes) RPT_SHADE_PUNCTUAL_ARG(, pl.lights, pl.n, pl.q));
            if (NEE != RPT_NEE_NONE) count_elided(&n_elided, elided);
            shade_emit<NEE>(q, push_scratch, slot, to_sky, emit_shadow, sh_o, sh_d, sh_c);
        }
    } else {
        const uint32_t slot = blockIdx.x * RPT_BLOCK + threadIdx.x;
        float2 hw = make_float2(0.0f, __uint_as_float(HIT_PARKED));
        if (slot < st.n_slots) hw = st.hit[slot];
        const uint32_t hit_tri = __float_as_uint(hw.y);
        const bool active = hit_tri < HIT_IDLE || hit_tri == HIT_MISS;        /* traversed in this iteration */
        bool to_sky = false, emit_shadow = false, elided = false;
        float4 sh_o = make_float4(0, 0, 0, 0), sh_d = sh_o, sh_c = sh_o;
        shade_slot<NEE, TEXTURED, false, RPT_SHADE_MODELS, RPT_SHADE_VOLUMES, RPT_SHADE_PUNCTUAL>(sc, st, q, cfg, stats, slot, hw, active, to_sky, emit_shadow, sh_o, sh_d, sh_c, first_paths, n_samples, elided, last_iteration RPT_SHADE_MODELS_ARG(, models) RPT_SHADE_VOLUMES_ARG(, volumes) RPT_SHADE_PUNCTUAL_ARG(, pl.lights, pl.n, pl.q));
        if (NEE != RPT_NEE_NONE) count_elided(&n_elided, elided);
        shade_emit<NEE>(q, push_scratch, slot, to_sky, emit_shadow, sh_o, sh_d, sh_c);
    }
    if (NEE != RPT_NEE_NONE) {
        /* one sharded, non-returning atomic per workgroup (element 1 of the shard's line: element 0 counts extension rays) */
        __syncthreads();
        if (threadIdx.x == 0u && n_elided != 0u) atomicAdd(&q.ray_shards[(blockIdx.x % RPT_STAT_SHARDS) * RPT_STAT_STRIDE + 1u], (unsigned long long)n_elided);
    }
}
