/*
 * k_complete_body.h — the text of the completion kernels, compiled once per build (as k_traverse_shadow_kernels.h is by rpt_traverse.hip):
 *   RPT_COMPLETE_KERNEL k_complete,              RPT_MOM(...) nothing       the kernel every context launches by default — a plain kernel under that name
 *   RPT_COMPLETE_KERNEL k_complete_moments,      RPT_MOM(...) its argument  with the moments record (rpt_set_moments): one more pointer argument
 *   RPT_COMPLETE_KERNEL k_lens_complete, k_lens_complete_moments            the same two with RPT_LENS(...) its argument — one more argument, the lens — and
 *                                                                           RPT_COMPLETE_START the lens's start of a path (rpt_lens.hip, rpt_set_camera_lens)
 * RPT_COMPLETE_DIRECT_ROWS and RPT_COMPLETE_RESTART_ROWS name the two helpers of the build that hold its macros; RPT_COMPLETE_START(st, cfg, slot, n, offset, todo_after)
 * is how a finished slot starts its next sample (k_complete.h: k_path.h start_path).  No include guard: the includer defines the six macros around each inclusion.
 */
/* pass 2 at q_shift = 0 (every shipped scene): row k of the chunk IS sample k of its 64 pixels with the lane's own pixel in its own lane — nothing to
 * transpose, no tile: G rows in flight, added in order straight from the registers; finished slots (k < n_done: the prefix) that owe nothing go idle.
 * `rad_bits` (own_rad, pass 1): bit i says that the lane's slot k0 + i is HIT_DONE and has a radiance record; a finished slot without one (HIT_DONE_ZERO) adds
 * (+0, +0, +0) and owes nothing.  Only the lanes with a record load: a row that has none issues no load. */
template <uint32_t G>
__device__ __forceinline__ bool RPT_COMPLETE_DIRECT_ROWS(const DevState &st, uint32_t base, uint32_t k0, uint32_t lane, bool ok, uint32_t n_done, uint32_t rad_bits,
                                                         float4 &acc RPT_MOM(, float4 &mom)) {
    float rx[G], ry[G], rz[G], rw[G];
    bool restart = false;
#pragma unroll
    for (uint32_t i = 0u; i < G; ++i) {
        float4 r = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0u));
        if (ok && k0 + i < n_done && ((rad_bits >> i) & 1u) != 0u) r = st.rad[base + ((k0 + i) << 6) + lane];
        rx[i] = r.x; ry[i] = r.y; rz[i] = r.z; rw[i] = r.w;
    }
#pragma unroll
    for (uint32_t i = 0u; i < G; ++i) {
        const bool mine = ok && k0 + i < n_done;
        if (mine) { acc.x += rx[i]; acc.y += ry[i]; acc.z += rz[i]; acc.w += 1.0f; }
        RPT_MOM(if (mine) mo_add(mom, rx[i], ry[i], rz[i]);)
        const uint32_t todo = __float_as_uint(rw[i]);
        if (mine && todo == 0u) st.hit[base + ((k0 + i) << 6) + lane] = make_float2(0.0f, __uint_as_float(HIT_IDLE));      /* (written out: through set_hit_word this unrolled loop compiles to other code) */
        restart = restart || rpt_ballot(mine && todo != 0u) != 0ull;
    }
    return restart;
}
/* the finished slots of a block that owe another sample start it (lib.rs:36-60) — never in the one completion of a batch of known length.  From the tile
 * (the record's .w is what the slot owes), row by row; slot k takes the samples k, k + S, ... */
__device__ __forceinline__ bool RPT_COMPLETE_RESTART_ROWS(const DevState &st, const DevConfig &cfg, uint32_t base, uint32_t kb, uint32_t rows, uint32_t rows_log, uint32_t lane,
                                                      const float4 *tile, const unsigned long long *row_done, unsigned long long ok_mask, uint32_t new_n, uint32_t rng_offset RPT_LENS(, const DevLens &lens)) {
    bool started = false;
#pragma unroll 1
    for (uint32_t t = 0u; t < rows; ++t) {
        const uint32_t slot = complete_block_slot(st, base, kb, t, rows, rows_log, lane), p = slot_pix(st, slot) & 63u, k = slot_k(st, slot);
        const uint32_t todo = __float_as_uint(tile[(k - kb) * RPT_COMPLETE_PITCH + p].w);
        const bool mine = ((row_done[(slot - base) >> 6] >> lane) & 1ull) != 0ull && ((ok_mask >> p) & 1ull) != 0ull && todo != 0u;
        const uint32_t n_of = (uint32_t)__shfl((int)new_n, (int)p, RPT_WAVE), offset_of = (uint32_t)__shfl((int)rng_offset, (int)p, RPT_WAVE);
        if (mine) {
            RPT_COMPLETE_START(st, cfg, slot, n_of + k, offset_of, todo - 1u);
            started = true;
        }
    }
    return started;
}
__global__ __launch_bounds__(RPT_WAVE) void RPT_COMPLETE_KERNEL(DevState st, DevQueues q, DevConfig cfg, uint32_t iteration, uint32_t final_pass,
                                                                DevStats *stats RPT_MOM(, float4 *moments /* n_pixels records beside st.accum */) RPT_LENS(, DevLens lens)) {
    /* a surplus launch of the run-ahead returns at once (grid-uniform) — but not the one completion of a batch of known length:
     * "drained" there only says that no RAY was left in an earlier iteration, the finished samples still wait to be added */
    if (!final_pass && q.count[Q_DRAINED] != 0u) return;
    extern __shared__ float4 complete_lds[];
    const uint32_t gs = st.group_shift, qs = st.q_shift, S = 1u << gs, rows = complete_rows(S);
    float4 *tile = complete_lds;
    unsigned long long *row_done = reinterpret_cast<unsigned long long *>(complete_lds + rows * RPT_COMPLETE_PITCH);
    /* which slots are HIT_DONE, whose radiance record pass 2 loads: per lane a byte for every eight rows (q_shift = 0 has neither tile nor row_done:
     * complete_lds_bytes).  (In registers they are 256 bits per lane at S = 256, eight VGPRs, and k_complete_moments has 94 of the 96 it is held to.) */
    uint8_t *own_rad = qs == 0u ? reinterpret_cast<uint8_t *>(complete_lds) : reinterpret_cast<uint8_t *>(row_done + S);
    const uint32_t lane = threadIdx.x, base = blockIdx.x << (6u + gs), pix = (blockIdx.x << 6) | lane;
    const bool in_image = pix < st.n_pixels;
    /* the rows that hold this lane's pixel (row >> (gs - qs) == its group), and where its Q slots sit in such a row's ballots */
    const uint32_t my_group = lane >> (6u - qs), my_shift = (lane & ((64u >> qs) - 1u)) << qs;
    const unsigned long long q_mask = (1ull << (1u << qs)) - 1ull;             /* (Q <= 32) */
    uint32_t n_done = 0u, n_busy = 0u, top = 0u;
    bool nothing_to_do = false;
    if (S >= 8u) {
        for (uint32_t j0 = 0u; j0 < S && !nothing_to_do; j0 += 8u) {
            complete_status_rows<8>(st, base, j0, lane, row_done, own_rad, my_group, my_shift, q_mask, n_done, n_busy, top);
            /* between the iterations of a call whose slots take several samples most pixels have a sample in flight: nothing to do for the chunk */
            nothing_to_do = !final_pass && rpt_ballot(in_image && n_busy == 0u) == 0ull;
        }
    } else if (S == 4u) complete_status_rows<4>(st, base, 0u, lane, row_done, own_rad, my_group, my_shift, q_mask, n_done, n_busy, top);
    else complete_status_rows<2>(st, base, 0u, lane, row_done, own_rad, my_group, my_shift, q_mask, n_done, n_busy, top);
    if (nothing_to_do) return;
    const bool ok = in_image && n_busy == 0u && n_done != 0u && top == n_done;
    if (final_pass && in_image && (n_busy != 0u || top != n_done)) {
        /* the one completion of a batch of known length found a sample still in flight: the bound on its iterations was wrong (must never
         * happen; rpt_wait / rpt_render report it) — or finished slots that are no prefix.  Counted like k_check_drained would: slots not idle. */
        atomicAdd(&stats->undrained, (unsigned long long)(n_done + n_busy));
    }
    const unsigned long long ok_mask = rpt_ballot(ok);
    bool started = false;
    if (ok_mask != 0ull) {
        float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        RPT_MOM(float4 mom = make_float4(0.0f, 0.0f, 0.0f, 0.0f);)
        uint2 rs = make_uint2(0u, 0u);
        if (ok) { acc = st.accum[pix]; rs = st.rng[pix]; }
        RPT_MOM(if (ok) mom = moments[pix];)
        const uint32_t new_n = rs.x + n_done;
        uint32_t most = ok ? n_done : 0u;                                   /* the chunk's longest prefix (wave-uniform) */
        for (uint32_t o = 32u; o != 0u; o >>= 1) { const uint32_t other = (uint32_t)__shfl_xor((int)most, (int)o, RPT_WAVE); most = other > most ? other : most; }
        const uint32_t rows_log = 31u - (uint32_t)__clz((int)rows);
        __syncthreads();                                                    /* row_done, own_rad written */
        if (qs == 0u) {
            const uint32_t G = S >= 8u ? 8u : S;
            for (uint32_t k0 = 0u; k0 < most; k0 += G) {
                bool restart;
                const uint32_t rad_bits = own_rad[(k0 >> 3) * RPT_WAVE + lane];        /* (k0 is a multiple of 8, or 0 with G = S < 8) */
                if (G == 8u) restart = RPT_COMPLETE_DIRECT_ROWS<8>(st, base, k0, lane, ok, n_done, rad_bits, acc RPT_MOM(, mom));
                else if (G == 4u) restart = RPT_COMPLETE_DIRECT_ROWS<4>(st, base, k0, lane, ok, n_done, rad_bits, acc RPT_MOM(, mom));
                else restart = RPT_COMPLETE_DIRECT_ROWS<2>(st, base, k0, lane, ok, n_done, rad_bits, acc RPT_MOM(, mom));
                if (restart) {                                              /* (never in the one completion of a batch of known length) */
#pragma unroll 1
                    for (uint32_t k = k0; k < k0 + G; ++k) {
                        const uint32_t slot = base + (k << 6) + lane;
                        const bool has_rad = ok && k < n_done && ((rad_bits >> (k - k0)) & 1u) != 0u;
                        const uint32_t todo = has_rad ? __float_as_uint(st.rad[slot].w) : 0u;
                        if (todo != 0u) {
                            RPT_COMPLETE_START(st, cfg, slot, new_n + k, rs.y, todo - 1u);      /* slot k takes the samples k, k + S, ... */
                            started = true;
                        }
                    }
                }
            }
        } else
        for (uint32_t kb = 0u; kb < most; kb += rows) {
            /* the rows that hold samples [kb, kb + rows) of all 64 pixels: for every pixel group, rows >> qs consecutive rows */
            bool restart = false;
            const uint32_t rad_bits = complete_block_rad_bits(st, base, kb, rows, rows_log, lane, own_rad);
            if (rows >= 8u) {
                for (uint32_t t0 = 0u; t0 < rows; t0 += 8u) restart |= complete_stage_rows<8>(st, base, kb, t0, rows, rows_log, lane, tile, row_done, rad_bits, ok_mask);
            } else if (rows == 4u) restart = complete_stage_rows<4>(st, base, kb, 0u, rows, rows_log, lane, tile, row_done, rad_bits, ok_mask);
            else restart = complete_stage_rows<2>(st, base, kb, 0u, rows, rows_log, lane, tile, row_done, rad_bits, ok_mask);
            __syncthreads();
            const uint32_t here = most - kb < rows ? most - kb : rows;
            for (uint32_t kl = 0u; kl < here; ++kl) {
                const float4 r = tile[kl * RPT_COMPLETE_PITCH + lane];
                if (ok && kb + kl < n_done) { acc.x += r.x; acc.y += r.y; acc.z += r.z; acc.w += 1.0f; }
                RPT_MOM(if (ok && kb + kl < n_done) mo_add(mom, r.x, r.y, r.z);)
            }
            if (restart) started |= RPT_COMPLETE_RESTART_ROWS(st, cfg, base, kb, rows, rows_log, lane, tile, row_done, ok_mask, new_n, rs.y RPT_LENS(, lens));
            __syncthreads();
        }
        if (ok) {
            st.accum[pix] = acc;
            rs.x = new_n;
            st.rng[pix] = rs;
            RPT_MOM(moments[pix] = mom;)
        }
    }
    /* tell the host that new samples were started (one plain store per wave, every writer stores 1) */
    const unsigned long long any = rpt_ballot(started);
    if (any != 0ull && lane == (uint32_t)__ffsll((long long)any) - 1u) raise_flag(&q.count[Q_REGEN0 + (iteration & 1u) * Q_LINE]);
}
