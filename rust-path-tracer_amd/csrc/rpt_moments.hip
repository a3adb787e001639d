/*
 * rpt_moments.hip — per-pixel sample moments behind the C ABI (include/rpt/rpt.h rpt_set_moments, rpt_moments, rpt_read_moments, rpt_read_noise,
 * rpt_noise_count, rpt_render_to_noise) and the host build of the noise estimate (rpt_debug.h rpt_debug_noise_host).  The record itself is kept by the
 * completion kernel of a context with moments on (k_complete.h k_complete_moments, launched by rpt_hip.hip); here are its life cycle, the read-outs
 * (k_image_order.h rpt_read_out), the count kernel and the render loop that stops at a noise target.  Arithmetic: k_moments.h.
 */
#include <chrono>
#include <vector>

#include "rpt_ctx.h"
#include "k_image_order.h"
#include "k_moments.h"

namespace {

/* counts[0] += pixels, [1] += measured, [2] += measured with !(rel <= threshold): one ballot per wave and count, one integer atomic per wave and
 * non-zero count — integers, so the result does not depend on the order the waves arrive in */
__global__ __launch_bounds__(RPT_BLOCK) void k_noise_count(const float4 *moments, uint32_t n_pixels, float threshold, unsigned long long *counts) {
    const uint32_t s = blockIdx.x * RPT_BLOCK + threadIdx.x;
    const bool in_range = s < n_pixels;
    bool measured = false, above = false;
    if (in_range) {
        const float4 m = moments[s];
        measured = mo_measured(m);
        above = measured && noise_above(noise_rel(m), threshold);
    }
    const unsigned long long mi = rpt_ballot(in_range), mm = rpt_ballot(measured), ma = rpt_ballot(above);
    if ((threadIdx.x & (RPT_WAVE - 1u)) == 0u) {
        if (mi != 0ull) atomicAdd(&counts[0], (unsigned long long)__popcll(mi));
        if (mm != 0ull) atomicAdd(&counts[1], (unsigned long long)__popcll(mm));
        if (ma != 0ull) atomicAdd(&counts[2], (unsigned long long)__popcll(ma));
    }
}

int need_moments(rpt_ctx *c, const char *who) {
    if (!c->moments_on) { c->error = std::string(who) + ": moments are off (rpt_set_moments(ctx, 1) first)"; return RPT_EINVAL; }
    if (!c->has_config || !c->has_state) { c->error = std::string(who) + ": no config"; return RPT_EINVAL; }
    return RPT_OK;
}

bool bad_threshold(float t) { return !(t >= 0.0f); }       /* negative or NaN (+inf is a threshold: nothing is above it but a NaN) */

/* the count on the context's stream behind whatever is enqueued, one wait, 24 bytes back */
int count_impl(rpt_ctx *c, float threshold, rpt_noise_counts *out) {
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->noise_counts.p) HIP_TRY(c, c->noise_counts.alloc(3));
    HIP_TRY(c, hipMemsetAsync(c->noise_counts.p, 0, 3 * sizeof(unsigned long long), c->stream));
    if (c->n_pixels) {
        k_noise_count<<<rpt_blocks(c->n_pixels), RPT_BLOCK, 0, c->stream>>>(c->moments.p, c->n_pixels, threshold, c->noise_counts.p);
        HIP_TRY(c, hipGetLastError());
    }
    RPT_TRY(rpt_wait(c));                /* (also verifies that asynchronous batches drained) */
    unsigned long long counts[3];
    HIP_TRY(c, hipMemcpy(counts, c->noise_counts.p, sizeof(counts), hipMemcpyDeviceToHost));
    out->pixels = counts[0]; out->measured = counts[1]; out->above = counts[2];
    return RPT_OK;
}

}  // namespace

/* The loop of rpt_render_to_noise / rpt_multi_render_to_noise over "render n more samples" and "count": batches of batch_samples clipped to max_samples, a
 * count after every batch from min_samples on, converged when every pixel is measured and at most max_above are above. */
template <typename Render, typename Count>
static int render_to_noise_loop(const rpt_noise_target &t, rpt_noise_result *out, Render render, Count count) {
    const auto t0 = std::chrono::steady_clock::now();
    rpt_noise_result res{};
    bool counted = false;
    while (res.samples_rendered < t.max_samples) {
        const uint32_t left = t.max_samples - res.samples_rendered, n = t.batch_samples < left ? t.batch_samples : left;
        RPT_TRY(render(n));
        res.samples_rendered += n;
        if (res.samples_rendered < t.min_samples) continue;
        RPT_TRY(count(&res.counts));
        counted = true;
        if (res.counts.measured == res.counts.pixels && res.counts.above <= t.max_above) { res.converged = 1u; break; }
    }
    if (!counted) RPT_TRY(count(&res.counts));       /* (max_samples = 0: the state as it is) */
    res.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = res;
    return RPT_OK;
}

int rpt_noise_check_target(const rpt_noise_target &t, std::string &error, const char *who) {
    if (t.batch_samples == 0u) { error = std::string(who) + ": batch_samples must be > 0"; return RPT_EINVAL; }
    if (t.max_samples < t.min_samples) { error = std::string(who) + ": max_samples must be >= min_samples"; return RPT_EINVAL; }
    if (bad_threshold(t.threshold)) { error = std::string(who) + ": threshold must be >= 0"; return RPT_EINVAL; }
    return RPT_OK;
}

int rpt_moments_reset(rpt_ctx *c) {
    if (!c->moments_on) return RPT_OK;
    if (c->moments.n != c->n_pixels) HIP_TRY(c, c->moments.alloc(c->n_pixels));
    if (c->n_pixels) HIP_TRY(c, hipMemsetAsync(c->moments.p, 0, (size_t)c->n_pixels * sizeof(float4), c->stream));
    return RPT_OK;
}

/* rpt_multi_render_to_noise (rpt_comm.hip owns rpt_multi): the same loop over its render and count */
int rpt_render_to_noise_with(const rpt_noise_target *target, rpt_noise_result *out, std::string &error, int (*render)(void *, uint32_t), int (*count)(void *, float, rpt_noise_counts *),
                             void *who) {
    RPT_TRY(rpt_noise_check_target(*target, error, "rpt_render_to_noise"));
    const float threshold = target->threshold;
    return render_to_noise_loop(*target, out, [=](uint32_t n) { return render(who, n); }, [=](rpt_noise_counts *k) { return count(who, threshold, k); });
}

extern "C" {

int rpt_set_moments(rpt_ctx *c, uint32_t on) {
    if (!c) return RPT_EINVAL;
    if (on == 0u && rpt_comm_gather_moments_on(c)) {   /* (a rank's message holds the record: its length must not depend on anything but the setting) */
        c->error = "rpt_set_moments: the gather carries the moments (rpt_gather_set_moments(ctx, 0) first)";
        return RPT_EINVAL;
    }
    if (c->has_state) RPT_TRY(rpt_wait(c));          /* batches enqueued so far keep the completion kernel they were enqueued with */
    if (on == 0u) {
        c->moments_on = false;
        c->moments.release();
        return RPT_OK;
    }
    if (c->moments_on) return RPT_OK;                /* on already: the record stays */
    c->moments_on = true;
    if (!c->has_state) return RPT_OK;                /* (allocated with the pixel state, by rpt_set_config) */
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = rpt_moments_reset(c);
    if (rc) { c->moments_on = false; c->moments.release(); }
    return rc;
}

int rpt_moments(rpt_ctx *c, uint32_t *on_out) {
    if (!c || !on_out) return RPT_EINVAL;
    *on_out = c->moments_on ? 1u : 0u;
    return RPT_OK;
}

int rpt_read_moments(rpt_ctx *c, float *out_xyzw) {
    if (!c || !out_xyzw) return RPT_EINVAL;
    RPT_TRY(need_moments(c, "rpt_read_moments"));
    return rpt_read_out(c, PixelCopy<float4>{c->moments.p, nullptr}, out_xyzw);
}

int rpt_read_noise(rpt_ctx *c, float *rel_out) {
    if (!c || !rel_out) return RPT_EINVAL;
    RPT_TRY(need_moments(c, "rpt_read_noise"));
    return rpt_read_out(c, PixelNoise{c->moments.p, nullptr}, rel_out);
}

int rpt_noise_count(rpt_ctx *c, float threshold, rpt_noise_counts *out) {
    if (!c || !out) return RPT_EINVAL;
    RPT_TRY(need_moments(c, "rpt_noise_count"));
    if (bad_threshold(threshold)) { c->error = "rpt_noise_count: threshold must be >= 0"; return RPT_EINVAL; }
    return count_impl(c, threshold, out);
}

int rpt_render_to_noise(rpt_ctx *c, const rpt_noise_target *target, rpt_noise_result *out) {
    if (!c || !target || !out) return RPT_EINVAL;
    RPT_TRY(rpt_noise_check_target(*target, c->error, "rpt_render_to_noise"));
    if (!c->has_scene || !c->has_config || !c->has_state) { c->error = "scene, config and reset must precede rpt_render_to_noise"; return RPT_EINVAL; }
    RPT_TRY(rpt_set_moments(c, 1u));
    const float threshold = target->threshold;
    return render_to_noise_loop(*target, out, [c](uint32_t n) { return rpt_render_async(c, n); }, [c, threshold](rpt_noise_counts *k) { return count_impl(c, threshold, k); });
}

/* noise_rel and the counts of rpt_noise_count on the host: the loop the kernels above are, over the same RPT_HD functions */
int rpt_debug_noise_host(const float *moments_xyzw, size_t n, float threshold, float *rel_out, rpt_noise_counts *counts_out) {
    if (!moments_xyzw && n != 0) return RPT_EINVAL;
    if (bad_threshold(threshold)) { rpt_create_error() = "rpt_debug_noise_host: threshold must be >= 0"; return RPT_EINVAL; }
    rpt_noise_counts k{};
    for (size_t i = 0; i < n; ++i) {
        const float4 m = make_float4(moments_xyzw[4 * i], moments_xyzw[4 * i + 1], moments_xyzw[4 * i + 2], moments_xyzw[4 * i + 3]);
        const float rel = noise_rel(m);
        if (rel_out) rel_out[i] = rel;
        k.pixels += 1;
        if (mo_measured(m)) { k.measured += 1; if (noise_above(rel, threshold)) k.above += 1; }
    }
    if (counts_out) *counts_out = k;
    return RPT_OK;
}

}  // extern "C"
