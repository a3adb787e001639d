/*
 * rpt_adaptive.hip — rendering chosen pixels behind the C ABI (include/rpt/rpt.h rpt_render_pixels, rpt_render_adaptive, rpt_render_adaptive_window,
 * rpt_adaptive_mask, rpt_counts_uniform) and the host builds of the selection (rpt_debug.h rpt_debug_adaptive_select_host, rpt_debug_adaptive_window_host).  A masked pass = select (flags, count per workgroup, scan), ONE small read-back
 * (how many pixels were selected), gather of their records into the context's compact arrays, the unchanged pipeline on that view of the context
 * (rpt_hip.hip rpt_render_view), scatter back — all on the context's stream.  Kernels and the selection rule: k_adaptive.h.
 */
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "rpt_ctx.h"
#include "k_image_order.h"
#include "k_adaptive.h"

static_assert(sizeof(AdResult) == 5 * sizeof(unsigned long long), "AdaptiveState::result is sized and zeroed as five 64-bit words");
static_assert(sizeof(AdTile) == 4 * sizeof(uint32_t), "AdaptiveState::tiles holds rpt_build_tile_table's four words per tile");

namespace {

uint32_t padded64(uint32_t n) { return (n + 63u) & ~63u; }

template <typename T> int grow(rpt_ctx *c, DevBuf<T> &b, size_t n) {
    if (b.n >= n) return RPT_OK;
    HIP_TRY(c, b.alloc(n));
    return RPT_OK;
}

int need_ready(rpt_ctx *c, const char *who) {
    if (!c->has_scene || !c->has_config || !c->has_state || !c->has_seeds) { c->error = std::string("scene, config and reset must precede ") + who; return RPT_EINVAL; }
    return RPT_OK;
}

/* Slots per pixel a view of n_active pixels may keep busy: the largest power of two <= RPT_MAX_SAMPLES_IN_FLIGHT whose slots, for the padded view, fit in
 * what a whole-image call of this context may allocate (max_slots) — so the path state never grows beyond that.  rpt_set_samples_in_flight(n > 0) holds for
 * the view as it holds for the image (n_active <= n_pixels: the context's own shift always fits). */
uint32_t view_max_shift(const rpt_ctx *c, uint32_t n_active) {
    if (c->samples_in_flight_request > 0) return c->max_group_shift;
    uint32_t shift = c->max_group_shift;
    while ((1u << (shift + 1u)) <= RPT_MAX_SAMPLES_IN_FLIGHT && ((uint64_t)padded64(n_active) << (shift + 1u)) <= c->max_slots) shift += 1u;
    return shift;
}

AdPixels own_pixels(rpt_ctx *c) { return AdPixels{c->pixel_xy.p, c->rng.p, c->accum.p, c->moments_on ? c->moments.p : nullptr}; }

uint64_t tiles_key(const rpt_ctx *c) { return (uint64_t)c->cfg.c.width | (uint64_t)c->cfg.c.height << 16 | (uint64_t)c->rank << 32 | (uint64_t)c->world << 48; }

}  // namespace

/* flags, workgroup counts and their scan, enqueued on the context's stream behind whatever is there */
int rpt_adaptive_select(rpt_ctx *c, const uint8_t *mask, const rpt_noise_target *target, uint32_t radius) {
    HIP_TRY(c, hipSetDevice(c->device));
    AdaptiveState &a = c->ad;
    const uint32_t n = c->n_pixels, blocks = rpt_blocks(n);
    const bool window = !mask && radius != 0u;
    if (window && radius > RPT_ADAPTIVE_MAX_RADIUS) { c->error = "adaptive selection: radius beyond RPT_ADAPTIVE_MAX_RADIUS (internal error)"; return RPT_EHIP; }
    if (a.flags.n < n || a.wg_count.n < blocks || !a.result.p || (window && a.tiles_key != tiles_key(c))) {
        if (c->async_pending) RPT_TRY(rpt_wait(c));          /* (an enqueued pass still reads the arrays that are about to go) */
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        RPT_TRY(grow(c, a.flags, n)); RPT_TRY(grow(c, a.wg_count, blocks)); RPT_TRY(grow(c, a.wg_offset, blocks));
        RPT_TRY(grow(c, a.result, sizeof(AdResult) / sizeof(unsigned long long)));
        if (window && a.tiles_key != tiles_key(c)) {
            /* the tile table of this size and partition (released with the pixel state, so a resize or another partition builds it again) */
            std::vector<uint32_t> table;
            rpt_build_tile_table(c->cfg.c.width, c->cfg.c.height, c->rank, c->world, table);
            a.tiles_key = 0;
            a.n_tiles = (uint32_t)(table.size() / 4u);
            uint32_t covered = 0;
            for (uint32_t t = 0; t < a.n_tiles; ++t) covered += table[4u * t + 1u];
            if (covered != n) { c->error = "adaptive selection: the tile table does not cover the owned pixels (internal error)"; return RPT_EHIP; }
            RPT_TRY(grow(c, a.tiles, table.size()));
            if (!table.empty()) HIP_TRY(c, hipMemcpy(a.tiles.p, table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            a.tiles_key = tiles_key(c);
        }
    }
    AdResult *res = reinterpret_cast<AdResult *>(a.result.p);
    HIP_TRY(c, hipMemsetAsync(res, 0, sizeof(AdResult), c->stream));
    if (n == 0u) return RPT_OK;
    if (mask) {
        /* the caller's row-major mask goes up as it is, as the seeds of rpt_reset do: a synchronous copy (complete when it returns) into the context's own
         * staging buffer, which no kernel is reading — every earlier select was waited for by the read of its result */
        const size_t whole = (size_t)c->cfg.c.width * c->cfg.c.height;
        RPT_TRY(grow(c, a.mask, whole));
        HIP_TRY(c, hipMemcpy(a.mask.p, mask, whole, hipMemcpyHostToDevice));
        k_ad_count<<<blocks, RPT_BLOCK, 0, c->stream>>>(AdMaskSel{c->pixel_xy.p, a.mask.p, c->cfg.c.width}, n, a.flags.p, a.wg_count.p, res);
    } else if (!window) {
        k_ad_count<<<blocks, RPT_BLOCK, 0, c->stream>>>(AdNoiseSel{c->moments.p, target->threshold, (float)target->batch_samples, (float)target->max_samples}, n, a.flags.p, a.wg_count.p, res);
    } else {
        /* the window rule: a workgroup per owned tile writes the flags and the counts; the compaction reads the flags it wrote */
        k_ad_window<<<a.n_tiles, RPT_BLOCK, 0, c->stream>>>(reinterpret_cast<const AdTile *>(a.tiles.p), c->pixel_xy.p, c->moments.p, n, target->threshold, (float)target->batch_samples,
                                                           (float)target->max_samples, radius, a.flags.p, res);
        HIP_TRY(c, hipGetLastError());
        k_ad_count<<<blocks, RPT_BLOCK, 0, c->stream>>>(AdFlagSel{a.flags.p}, n, a.flags.p, a.wg_count.p, res);
    }
    HIP_TRY(c, hipGetLastError());
    k_ad_scan<<<1, RPT_BLOCK, 0, c->stream>>>(a.wg_count.p, blocks, a.wg_offset.p, res);
    HIP_TRY(c, hipGetLastError());
    return RPT_OK;
}

/* the pass's one synchronisation: 4 bytes (a mask) or the whole record (a noise selection) */
int rpt_adaptive_selected(rpt_ctx *c, bool with_counts, rpt_adaptive_selection *out) {
    HIP_TRY(c, hipSetDevice(c->device));
    RPT_TRY(rpt_wait(c));                    /* (also verifies that asynchronous batches drained) */
    AdResult res{};
    HIP_TRY(c, hipMemcpy(&res, c->ad.result.p, with_counts ? sizeof(res) : sizeof(res.n_active), hipMemcpyDeviceToHost));
    c->ad.n_active = res.n_active;
    *out = rpt_adaptive_selection{res.n_active, ~res.z_min_inv, res.z_max, rpt_noise_counts{res.pixels, res.measured, res.above}};
    return RPT_OK;
}

int rpt_adaptive_pass(rpt_ctx *c, uint32_t n_samples, bool uniform_ok) {
    AdaptiveState &a = c->ad;
    const uint32_t n_active = a.n_active;
    a.n_active = 0u;                         /* (a selection is rendered once) */
    if (n_active == 0u || n_samples == 0u) return RPT_OK;
    if (n_active > c->n_pixels) { c->error = "masked pass: more pixels selected than owned (internal error)"; return RPT_EHIP; }
    /* every owned pixel: this IS a uniform call, and runs as one — the context's own arrays, its uniform sample count (uniform_ok: unless another rank of
     * the same image renders only some of its pixels in this pass, rpt_comm.hip) */
    if (n_active == c->n_pixels && uniform_ok) return rpt_render_async(c, n_samples);
    HIP_TRY(c, hipSetDevice(c->device));
    if (a.active.n < n_active || (c->moments_on && a.moments.n < n_active)) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        const uint32_t room = padded64(n_active);            /* (whole chunks of 64 pixels, as the view's slots are laid out) */
        RPT_TRY(grow(c, a.active, room)); RPT_TRY(grow(c, a.pixel_xy, room)); RPT_TRY(grow(c, a.rng, room)); RPT_TRY(grow(c, a.accum, room));
        if (c->moments_on) RPT_TRY(grow(c, a.moments, room));
    }
    const AdPixels whole = own_pixels(c), compact{a.pixel_xy.p, a.rng.p, a.accum.p, c->moments_on ? a.moments.p : nullptr};
    k_ad_scatter<<<rpt_blocks(c->n_pixels), RPT_BLOCK, 0, c->stream>>>(whole, c->n_pixels, a.flags.p, a.wg_offset.p, n_active, a.active.p, compact);
    HIP_TRY(c, hipGetLastError());
    const PixelView view{a.pixel_xy.p, a.rng.p, a.accum.p, compact.moments, n_active, view_max_shift(c, n_active)};
    RPT_TRY(rpt_render_view(c, n_samples, &view));
    k_ad_scatter_back<<<rpt_blocks(n_active), RPT_BLOCK, 0, c->stream>>>(compact, a.active.p, n_active, c->n_pixels, whole);
    HIP_TRY(c, hipGetLastError());
    c->counts_nonuniform = true;
    return RPT_OK;
}

int rpt_resolve_own(rpt_ctx *c, uint32_t tonemap_op, float *out_rgb) { return rpt_read_out(c, PixelResolveOwn{c->accum.p, tonemap_op, nullptr}, out_rgb); }

/* The loop of rpt_render_adaptive / rpt_multi_render_adaptive.  Uniform phase: min_samples exactly, in batches of at most batch_samples.  Then, before each
 * masked pass, select and count: converged when every pixel is measured and at most max_above are above the threshold; done, not converged, when the rule
 * selects nothing (every pixel still above has reached the cap); else batch_samples more for the selected pixels. */
int rpt_render_adaptive_with(const rpt_noise_target *target, rpt_adaptive_result *out, const rpt_adaptive_driver &driver, void *who) {
    const auto t0 = std::chrono::steady_clock::now();
    const rpt_noise_target &t = *target;
    rpt_adaptive_result res{};
    for (uint32_t done = 0; done < t.min_samples;) {
        const uint32_t left = t.min_samples - done, n = t.batch_samples < left ? t.batch_samples : left;
        uint64_t rendered = 0;
        RPT_TRY(driver.render(who, n, &rendered));
        res.pixel_samples += rendered;
        done += n;
    }
    for (;;) {
        rpt_adaptive_selection sel{};
        RPT_TRY(driver.select(who, target, &sel));
        res.counts = sel.counts;
        res.min_pixel_samples = sel.counts.pixels ? sel.z_min : 0u;
        res.max_pixel_samples = sel.z_max;
        if (sel.counts.measured == sel.counts.pixels && sel.counts.above <= t.max_above) { res.converged = 1u; break; }
        if (sel.n_active == 0u) break;
        RPT_TRY(driver.pass(who, t.batch_samples));
        res.passes += 1u;
        res.pixel_samples += (uint64_t)sel.n_active * t.batch_samples;
    }
    res.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = res;
    return RPT_OK;
}

int rpt_adaptive_mask_check(rpt_ctx *c, const rpt_noise_target *target, uint32_t radius, std::string &error, const char *who) {
    if (!target) { error = std::string(who) + ": null target"; return RPT_EINVAL; }
    RPT_TRY(rpt_noise_check_target(*target, error, who));
    if (radius > RPT_ADAPTIVE_MAX_RADIUS) { error = std::string(who) + ": radius must be <= RPT_ADAPTIVE_MAX_RADIUS (8)"; return RPT_EINVAL; }
    if (!c->has_scene || !c->has_config || !c->has_state || !c->has_seeds) { error = std::string("scene, config and reset must precede ") + who; return RPT_EINVAL; }
    if (!c->moments_on) { error = std::string(who) + ": moments are off (rpt_set_moments(ctx, 1) first)"; return RPT_EINVAL; }
    return RPT_OK;
}

extern "C" {

int rpt_render_pixels(rpt_ctx *c, const uint8_t *mask, uint32_t n_samples) {
    if (!c) return RPT_EINVAL;
    if (!mask) { c->error = "rpt_render_pixels: null mask"; return RPT_EINVAL; }
    RPT_TRY(need_ready(c, "rpt_render_pixels"));
    if (n_samples == 0u || c->n_pixels == 0u) return RPT_OK;
    rpt_adaptive_selection sel{};
    RPT_TRY(rpt_adaptive_select(c, mask, nullptr, 0u));
    RPT_TRY(rpt_adaptive_selected(c, false, &sel));
    return rpt_adaptive_pass(c, n_samples, true);
}

/* rpt_render_adaptive (radius 0) and rpt_render_adaptive_window: one loop, the selection differs */
static int render_adaptive(rpt_ctx *c, const rpt_noise_target *target, uint32_t radius, rpt_adaptive_result *out, const char *who) {
    if (!c || !target || !out) return RPT_EINVAL;
    RPT_TRY(rpt_noise_check_target(*target, c->error, who));
    if (radius > RPT_ADAPTIVE_MAX_RADIUS) { c->error = std::string(who) + ": radius must be <= RPT_ADAPTIVE_MAX_RADIUS (8)"; return RPT_EINVAL; }
    RPT_TRY(need_ready(c, who));
    RPT_TRY(rpt_set_moments(c, 1u));
    struct Who { rpt_ctx *c; uint32_t radius; } w{c, radius};
    const rpt_adaptive_driver driver = {
        [](void *who, uint32_t n, uint64_t *rendered) {
            rpt_ctx *c = static_cast<Who *>(who)->c;
            *rendered = (uint64_t)c->n_pixels * n;
            return rpt_render_async(c, n);
        },
        [](void *who, const rpt_noise_target *t, rpt_adaptive_selection *sel) {
            const Who *w = static_cast<Who *>(who);
            RPT_TRY(rpt_adaptive_select(w->c, nullptr, t, w->radius));
            return rpt_adaptive_selected(w->c, true, sel);
        },
        [](void *who, uint32_t n) { return rpt_adaptive_pass(static_cast<Who *>(who)->c, n, true); }};
    return rpt_render_adaptive_with(target, out, driver, &w);
}

int rpt_render_adaptive(rpt_ctx *c, const rpt_noise_target *target, rpt_adaptive_result *out) { return render_adaptive(c, target, 0u, out, "rpt_render_adaptive"); }

int rpt_render_adaptive_window(rpt_ctx *c, const rpt_noise_target *target, uint32_t radius, rpt_adaptive_result *out) {
    return render_adaptive(c, target, radius, out, "rpt_render_adaptive_window");
}

/* the flags of the selection the next pass of that call would make, read out as every per-pixel record is (k_image_order.h); nothing is rendered and the
 * selection is dropped: the flag bytes and the result record are scratch of the masked passes */
int rpt_adaptive_mask(rpt_ctx *c, const rpt_noise_target *target, uint32_t radius, uint8_t *mask_out, rpt_noise_counts *counts_out) {
    if (!c) return RPT_EINVAL;
    RPT_TRY(rpt_adaptive_mask_check(c, target, radius, c->error, "rpt_adaptive_mask"));
    if (!mask_out) { c->error = "rpt_adaptive_mask: null mask_out"; return RPT_EINVAL; }
    rpt_adaptive_selection sel{};
    RPT_TRY(rpt_adaptive_select(c, nullptr, target, radius));
    RPT_TRY(rpt_adaptive_selected(c, true, &sel));
    c->ad.n_active = 0u;
    if (counts_out) *counts_out = sel.counts;
    return rpt_read_out(c, PixelCopy<uint8_t>{c->ad.flags.p, nullptr}, mask_out);
}

int rpt_counts_uniform(rpt_ctx *c, uint32_t *uniform_out) {
    if (!c || !uniform_out) return RPT_EINVAL;
    *uniform_out = c->counts_nonuniform ? 0u : 1u;
    return RPT_OK;
}

/* the selection rule and the ordered compaction on the host: the loop the kernels of k_adaptive.h are, over the same RPT_HD function */
int rpt_debug_adaptive_select_host(const float *moments_xyzw, size_t n, float threshold, uint32_t batch_samples, uint32_t max_samples, uint8_t *flags_out, uint32_t *active_out,
                                   size_t *n_active_out) {
    if ((!moments_xyzw && n != 0) || n > 0xffffffffull) return RPT_EINVAL;
    if (!(threshold >= 0.0f)) { rpt_create_error() = "rpt_debug_adaptive_select_host: threshold must be >= 0"; return RPT_EINVAL; }
    size_t k = 0;
    for (size_t i = 0; i < n; ++i) {
        const float4 m = make_float4(moments_xyzw[4 * i], moments_xyzw[4 * i + 1], moments_xyzw[4 * i + 2], moments_xyzw[4 * i + 3]);
        const bool chosen = adaptive_selected(m, threshold, (float)batch_samples, (float)max_samples);
        if (flags_out) flags_out[i] = chosen ? 1u : 0u;
        if (chosen) {
            if (active_out) active_out[k] = (uint32_t)i;
            k += 1;
        }
    }
    if (n_active_out) *n_active_out = k;
    return RPT_OK;
}

/* the selection step alone, timed: HIP events on the context's stream around what rpt_adaptive_select enqueues (the result's memset, the flags, the counts per
 * workgroup, the scan), `repeats` times after one untimed round that makes the allocations; nothing is rendered and the selection is dropped */
int rpt_debug_adaptive_select_ms(rpt_ctx *c, const rpt_noise_target *target, uint32_t radius, uint32_t repeats, float *ms_out) {
    if (!c) return RPT_EINVAL;
    RPT_TRY(rpt_adaptive_mask_check(c, target, radius, c->error, "rpt_debug_adaptive_select_ms"));
    if (!ms_out || repeats == 0u) { c->error = "rpt_debug_adaptive_select_ms: no room for a time"; return RPT_EINVAL; }
    HIP_TRY(c, hipSetDevice(c->device));
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() { for (hipEvent_t v : e) if (v) (void)hipEventDestroy(v); }
    } ev;
    HIP_TRY(c, hipEventCreate(&ev.e[0])); HIP_TRY(c, hipEventCreate(&ev.e[1]));
    rpt_adaptive_selection sel{};
    RPT_TRY(rpt_adaptive_select(c, nullptr, target, radius));
    RPT_TRY(rpt_adaptive_selected(c, true, &sel));
    for (uint32_t k = 0; k < repeats; ++k) {
        HIP_TRY(c, hipEventRecord(ev.e[0], c->stream));
        RPT_TRY(rpt_adaptive_select(c, nullptr, target, radius));
        HIP_TRY(c, hipEventRecord(ev.e[1], c->stream));
        HIP_TRY(c, hipEventSynchronize(ev.e[1]));
        HIP_TRY(c, hipEventElapsedTime(&ms_out[k], ev.e[0], ev.e[1]));
    }
    RPT_TRY(rpt_adaptive_selected(c, true, &sel));
    c->ad.n_active = 0u;
    return RPT_OK;
}

/* the window rule on the host: the three steps of k_ad_window over every tile of a row-major image, on the same RPT_HD functions */
int rpt_debug_adaptive_window_host(const float *moments_xyzw, uint32_t width, uint32_t height, float threshold, uint32_t batch_samples, uint32_t max_samples, uint32_t radius,
                                   uint8_t *flags_out) {
    if (!moments_xyzw || !flags_out || !width || !height || width > 65535u || height > 65535u) return RPT_EINVAL;
    if (!(threshold >= 0.0f)) { rpt_create_error() = "rpt_debug_adaptive_window_host: threshold must be >= 0"; return RPT_EINVAL; }
    if (radius > RPT_ADAPTIVE_MAX_RADIUS) { rpt_create_error() = "rpt_debug_adaptive_window_host: radius must be <= RPT_ADAPTIVE_MAX_RADIUS (8)"; return RPT_EINVAL; }
    const auto record = [&](uint32_t x, uint32_t y) {
        const float *m = moments_xyzw + 4u * ((size_t)y * width + x);
        return make_float4(m[0], m[1], m[2], m[3]);
    };
    for (uint32_t ty = 0; ty < height; ty += RPT_TILE)
        for (uint32_t tx = 0; tx < width; tx += RPT_TILE) {
            const uint32_t w = std::min<uint32_t>(RPT_TILE, width - tx), h = std::min<uint32_t>(RPT_TILE, height - ty);
            unsigned long long rows[RPT_TILE] = {}, wide[RPT_TILE];
            for (uint32_t y = 0; y < h; ++y)
                for (uint32_t x = 0; x < w; ++x)
                    if (ad_above(record(tx + x, ty + y), threshold)) rows[y] |= 1ull << x;
            for (uint32_t y = 0; y < RPT_TILE; ++y) wide[y] = ad_dilate_row(rows[y], radius);
            for (uint32_t y = 0; y < RPT_TILE; ++y) rows[y] = ad_dilate_rows(wide, y, radius);
            for (uint32_t y = 0; y < h; ++y)
                for (uint32_t x = 0; x < w; ++x)
                    flags_out[(size_t)(ty + y) * width + tx + x] = ((rows[y] >> x) & 1ull) != 0ull && ad_fits(record(tx + x, ty + y), (float)batch_samples, (float)max_samples) ? 1u : 0u;
        }
    return RPT_OK;
}

}  // extern "C"
