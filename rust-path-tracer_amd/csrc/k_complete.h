/*
 * k_complete.h — the completion of sample generations (kernels/src/lib.rs:225-226: `output[i] += (radiance, 1)`, `rng[i].x += 1`), the one kernel that adds
 * finished samples to the accumulators.  Compiled in rpt_hip.hip.
 */
#ifndef RPT_K_COMPLETE_H
#define RPT_K_COMPLETE_H

#include "k_path.h"
#include "k_moments.h"

/* Completion of generations: ONE WAVE PER CHUNK of 64 pixels, lane = pixel.  When all S slots of a pixel are finished (HIT_DONE) or have
 * nothing left (HIT_IDLE) and at least one is finished, their radiances are added to the accumulator IN SLOT ORDER (= sample order,
 * kernels/src/lib.rs:225, src/trace.rs:295: the f32 sum order is part of the result), the pixel's rng.n advances by the number of samples
 * (lib.rs:226), and every finished slot starts its next sample (lib.rs:36-60) or goes idle.
 *
 * Every global access is a ROW of the chunk — 64 consecutive slots, one coalesced wave access — whatever the slot layout (k_common.h
 * slot_pix: a row is 64 pixels at one sample index for q_shift = 0, 64 / Q pixels x Q samples otherwise):
 *   pass 1  the hit words, row by row: two ballots per row tell every lane which of ITS pixel's slots are finished / still in flight;
 *   pass 2  q_shift = 0: a row is one sample of the chunk's 64 pixels, lane = pixel — eight rows in flight, added in order from the registers;
 *           q_shift > 0: the radiance records of up to 32 samples of all 64 pixels, row by row into an LDS tile [sample][pixel] (the transposition
 *           the layout needs), then every lane adds its pixel's column of the tile in sample order;
 *           either way the finished slots of a row go idle (or start their next sample) as the row passes.
 * Slot k takes the samples k, k + S, ... of a call, so within a generation the finished slots of a pixel are a PREFIX of its slots: the lane
 * keeps a count (checked against the highest finished slot), which is what lets S go beyond the 32 bits of a mask — up to 256 samples of a
 * pixel in flight (a rank that owns 1/8 of an image fills its launches with 8 x the samples per pixel).
 * History: round 2 completed inside the shade stage (a DPP chain across lanes, 0.45 ms of a DarkCornell batch); rounds 3-5 one THREAD per
 * pixel looping over its slots — coalesced only at q_shift = 0: 5.6 ms instead of 0.9 per 2048^2 x 32 slots on the large-scene layout.
 * A batch of known length (no slot takes a second sample) runs this once, after its last iteration; otherwise it follows every shade stage.
 * Two kernels share the text (k_complete_body.h, compiled twice): k_complete, and k_complete_moments for a context with moments on (rpt_set_moments), which adds
 * every sample it adds to the accumulator to the pixel's moments record too (k_moments.h mo_add) — from the same registers / tile column, in the same
 * order: one more float4 load and store per completing pixel, four VALU operations per sample. */
#define RPT_COMPLETE_ROWS 32u          /* samples of a pixel staged per pass */
#define RPT_COMPLETE_PITCH 65u         /* float4 per tile row: 64 pixels + 1 (the transposing stores of a q_shift > 0 row would share a bank) */
__host__ __device__ __forceinline__ uint32_t complete_rows(uint32_t S) { return S < RPT_COMPLETE_ROWS ? S : RPT_COMPLETE_ROWS; }
__host__ __device__ __forceinline__ size_t complete_lds_bytes(uint32_t S, uint32_t q_shift) {
    /* own_rad (a byte per lane and eight rows), and for q_shift > 0 the tile and row_done in front of it */
    return (size_t)((S + 7u) / 8u) * RPT_WAVE + (q_shift == 0u ? 0u : (size_t)complete_rows(S) * RPT_COMPLETE_PITCH * sizeof(float4) + (size_t)S * sizeof(unsigned long long));
}
/* pass 1 of k_complete for G consecutive rows of the chunk (G loads in flight): the row's "finished" ballot goes to LDS for pass 2, the lane
 * takes the bits of its own pixel out of the rows that hold it.
 * A finished slot is HIT_DONE (its radiance record was written) or HIT_DONE_ZERO (radiance +0, nothing owed, NO record: k_common.h).  Pass 2 loads the record
 * of the first kind only, so pass 1 also keeps which slots are HIT_DONE, in LDS: one byte per lane and eight rows, bit i = the lane's slot of row j0 + i
 * (own_rad: the call's rows are one such group, G <= 8 and j0 a multiple of 8) — a lane of pass 2 looks at the rows in the lane it looked at them here. */
template <uint32_t G>
__device__ __forceinline__ void complete_status_rows(const DevState &st, uint32_t base, uint32_t j0, uint32_t lane, unsigned long long *row_done, uint8_t *own_rad, uint32_t my_group, uint32_t my_shift, unsigned long long q_mask, uint32_t &n_done, uint32_t &n_busy, uint32_t &top) {
    const uint32_t gs = st.group_shift, qs = st.q_shift;
    uint32_t w[G];
#pragma unroll
    for (uint32_t i = 0u; i < G; ++i) w[i] = __float_as_uint(st.hit[base + ((j0 + i) << 6) + lane].y);
    uint32_t own = 0u;
#pragma unroll
    for (uint32_t i = 0u; i < G; ++i) {
        const uint32_t row = j0 + i;
        const bool has_rad = w[i] == HIT_DONE, done = has_rad || w[i] == HIT_DONE_ZERO;
        const unsigned long long md = rpt_ballot(done), mb = rpt_ballot(!done && w[i] != HIT_IDLE);
        if (qs != 0u && lane == 0u) row_done[row] = md;               /* (q_shift = 0: pass 2 needs no masks, the finished slots of a pixel are its first n_done) */
        own |= (has_rad ? 1u : 0u) << i;
        if ((row >> (gs - qs)) == my_group) {
            const uint32_t bits = (uint32_t)((md >> my_shift) & q_mask);
            n_done += (uint32_t)__popc(bits);
            n_busy += (uint32_t)__popc((uint32_t)((mb >> my_shift) & q_mask));
            if (bits != 0u) top = ((row & ((1u << (gs - qs)) - 1u)) << qs) + 32u - (uint32_t)__clz((int)bits);    /* (rows ascend: the last one wins) */
        }
    }
    own_rad[(j0 >> 3) * RPT_WAVE + lane] = (uint8_t)own;
}
/* Row t of a block of `rows` samples starting at sample kb: for every pixel group, rows >> qs consecutive rows of the chunk. */
__device__ __forceinline__ uint32_t complete_block_slot(const DevState &st, uint32_t base, uint32_t kb, uint32_t t, uint32_t rows, uint32_t rows_log, uint32_t lane) {
    const uint32_t gs = st.group_shift, qs = st.q_shift;
    const uint32_t g = t >> (rows_log - qs), jl = (kb >> qs) + (t & ((rows >> qs) - 1u));
    return base + (((g << (gs - qs)) | jl) << 6) + lane;
}
/* which rows of such a block hold a HIT_DONE slot in this lane: bit t = row t of the block, gathered from own_rad (one pass over the block's rows ahead of
 * its loads: a byte read per row inside complete_stage_rows kept eight more registers alive, 92 and 100 VGPRs) */
__device__ __forceinline__ uint32_t complete_block_rad_bits(const DevState &st, uint32_t base, uint32_t kb, uint32_t rows, uint32_t rows_log, uint32_t lane, const uint8_t *own_rad) {
    uint32_t bits = 0u;
#pragma unroll 1
    for (uint32_t t = 0u; t < rows; ++t) {
        const uint32_t row = (complete_block_slot(st, base, kb, t, rows, rows_log, lane) - base) >> 6;
        bits |= (((uint32_t)own_rad[(row >> 3) * RPT_WAVE + lane] >> (row & 7u)) & 1u) << t;
    }
    return bits;
}
/* pass 2 of k_complete for G rows of such a block (G loads in flight): the radiance records into the tile [sample - kb][pixel] — loaded by the HIT_DONE lanes
 * of a row only (rad_bits; a row without one issues no load), (+0, +0, +0, owes 0) for every other lane — the finished slots of the
 * completing pixels that owe nothing more marked idle.  Returns (wave-uniform) whether some finished slot owes another sample (complete_restart_rows). */
template <uint32_t G>
__device__ __forceinline__ bool complete_stage_rows(const DevState &st, uint32_t base, uint32_t kb, uint32_t t0, uint32_t rows, uint32_t rows_log, uint32_t lane, float4 *tile,
                                                    const unsigned long long *row_done, uint32_t rad_bits, unsigned long long ok_mask) {
    float rx[G], ry[G], rz[G], rw[G];              /* (scalars: an array of float4 stays in scratch behind its 16-byte copies) */
    uint32_t slot_of[G];
    bool restart = false;
#pragma unroll
    for (uint32_t i = 0u; i < G; ++i) {
        slot_of[i] = complete_block_slot(st, base, kb, t0 + i, rows, rows_log, lane);
        float4 r = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0u));
        if (((rad_bits >> (t0 + i)) & 1u) != 0u) r = st.rad[slot_of[i]];
        rx[i] = r.x; ry[i] = r.y; rz[i] = r.z; rw[i] = r.w;
    }
#pragma unroll
    for (uint32_t i = 0u; i < G; ++i) {
        const uint32_t slot = slot_of[i], p = slot_pix(st, slot) & 63u, k = slot_k(st, slot);
        tile[(k - kb) * RPT_COMPLETE_PITCH + p] = make_float4(rx[i], ry[i], rz[i], rw[i]);
        const bool mine = ((row_done[(slot - base) >> 6] >> lane) & 1ull) != 0ull && ((ok_mask >> p) & 1ull) != 0ull;
        const uint32_t todo = __float_as_uint(rw[i]);
        if (mine && todo == 0u) set_hit_word(st, slot, HIT_IDLE);
        restart = restart || rpt_ballot(mine && todo != 0u) != 0ull;
    }
    return restart;
}
/* The kernels: one text (k_complete_body.h: the kernel and the two helpers it calls that differ between the builds — the q_shift = 0 row helper and the q_shift > 0
 * restart) compiled twice here; RPT_MOM(...) there is its argument in the moments build and nothing in the plain one, RPT_LENS(...) is nothing in either and
 * RPT_COMPLETE_START is start_path, so the plain k_complete is compiled from the text it always had.  k_complete stays a plain kernel under that
 * name, not a template instantiation (tests/test_kernel_resources.py finds the completion kernels by the prefix "k_complete"); k_complete_moments is launched
 * instead of it by a context with moments on.  The moments pointer is an argument of that kernel, not a field of DevState, which every stage kernel takes:
 * no other kernel changes.  rpt_lens.hip compiles the text twice more for a context with an active lens: it defines RPT_COMPLETE_HELPERS_ONLY before it
 * includes this header, because the two kernels below are plain symbols of rpt_hip.hip. */
#ifndef RPT_COMPLETE_HELPERS_ONLY
#define RPT_LENS(...)
#define RPT_COMPLETE_START(...) start_path(__VA_ARGS__)
#define RPT_COMPLETE_KERNEL k_complete
#define RPT_COMPLETE_DIRECT_ROWS complete_direct_rows
#define RPT_COMPLETE_RESTART_ROWS complete_restart_rows
#define RPT_MOM(...)
#include "k_complete_body.h"
#undef RPT_COMPLETE_KERNEL
#undef RPT_COMPLETE_DIRECT_ROWS
#undef RPT_COMPLETE_RESTART_ROWS
#undef RPT_MOM
#define RPT_COMPLETE_KERNEL k_complete_moments
#define RPT_COMPLETE_DIRECT_ROWS complete_direct_rows_moments
#define RPT_COMPLETE_RESTART_ROWS complete_restart_rows_moments
#define RPT_MOM(...) __VA_ARGS__
#include "k_complete_body.h"
#undef RPT_COMPLETE_KERNEL
#undef RPT_COMPLETE_DIRECT_ROWS
#undef RPT_COMPLETE_RESTART_ROWS
#undef RPT_MOM
#undef RPT_COMPLETE_START
#undef RPT_LENS
#endif /* RPT_COMPLETE_HELPERS_ONLY */

#endif /* RPT_K_COMPLETE_H */
