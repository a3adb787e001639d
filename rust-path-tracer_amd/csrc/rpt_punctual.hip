/*
 * rpt_punctual.hip — punctual lights (include/rpt/rpt.h rpt_set_punctual_lights): the light records, and the punctual variant of the surface stage,
 * k_shade_punctual = the kernel text of k_shade (k_shade_body.h) with shade_slot<.., MODELS, VOLUMES, PUNCTUAL>.  A translation unit of its own, and the lights
 * one more argument of their own, as rpt_models.hip and rpt_volumes.hip have it: no kernel of the other units changes for it.  launch_iteration (rpt_hip.hip)
 * launches this variant in place of the other three when NEE is on and lights are set (or the test hook asks), so every route into the pipeline takes it; with
 * no lights, or with nee = 0 — a delta light is never met by a BSDF sample — the launch is the one made without this unit.
 */
#include <cmath>
#include <cstring>

#include "rpt_ctx.h"

#include "k_shade.h"

static_assert(sizeof(rpt_punctual_light) == 4 * sizeof(float4), "one host record, 64 bytes, becomes four float4 (k_punctual.h)");
static_assert(RPT_LIGHT_POINT == RPT_PUNCTUAL_POINT && RPT_LIGHT_SPOT == RPT_PUNCTUAL_SPOT && RPT_LIGHT_DIRECTIONAL == RPT_PUNCTUAL_DIRECTIONAL, "rpt.h and k_punctual.h name the same types");

/* (no occupancy asked of the compiler, as for k_shade_models and k_shade_volumes; the NEE_NONE instantiations are never launched: launch_iteration keeps the
 * other variants for nee = 0) */
#define RPT_SHADE_KERNEL k_shade_punctual
#define RPT_SHADE_MODELS true
#define RPT_SHADE_MODELS_ARG(...) __VA_ARGS__
#define RPT_SHADE_VOLUMES true
#define RPT_SHADE_VOLUMES_ARG(...) __VA_ARGS__
#define RPT_SHADE_PUNCTUAL true
#define RPT_SHADE_PUNCTUAL_ARG(...) __VA_ARGS__
#define RPT_SHADE_OCCUPANCY
#include "k_shade_body.h"
#undef RPT_SHADE_KERNEL
#undef RPT_SHADE_MODELS
#undef RPT_SHADE_MODELS_ARG
#undef RPT_SHADE_VOLUMES
#undef RPT_SHADE_VOLUMES_ARG
#undef RPT_SHADE_PUNCTUAL
#undef RPT_SHADE_PUNCTUAL_ARG
#undef RPT_SHADE_OCCUPANCY

template <int NEE, bool TEXTURED>
static void launch(rpt_ctx *c, uint32_t iteration, uint32_t blocks) {
    const uint4 *models = reinterpret_cast<const uint4 *>(c->material_models.p);
    const float4 *volumes = reinterpret_cast<const float4 *>(c->material_volumes.p);
    const DevPunctual pl{c->punctual_lights.p, (uint32_t)c->punctual_lights_host.size(), c->punctual_share};
    if (c->shade_compact) k_shade_punctual<NEE, TEXTURED, true><<<(c->n_slots + RPT_BLOCK * RPT_SHADE_ROUNDS - 1) / (RPT_BLOCK * RPT_SHADE_ROUNDS), RPT_BLOCK, 0, c->stream>>>(c->scene, c->state, c->queues, c->cfg, iteration, c->dev_stats.p, c->call_samples, models, volumes, pl);
    else k_shade_punctual<NEE, TEXTURED, false><<<blocks, RPT_BLOCK, 0, c->stream>>>(c->scene, c->state, c->queues, c->cfg, iteration, c->dev_stats.p, c->call_samples, models, volumes, pl);
}

/* (called for NEE modes 1 and 2 only) */
void rpt_launch_shade_punctual(rpt_ctx *c, uint32_t iteration, uint32_t blocks) {
    const bool tex = c->scene.textured != 0u;
    if (c->cfg.nee_mode == RPT_NEE_MIS) return tex ? launch<RPT_NEE_MIS, true>(c, iteration, blocks) : launch<RPT_NEE_MIS, false>(c, iteration, blocks);
    return tex ? launch<RPT_NEE_DIRECT, true>(c, iteration, blocks) : launch<RPT_NEE_DIRECT, false>(c, iteration, blocks);
}

/* rpt_upload_scene: the lights belong to the scene that was */
void rpt_punctual_lights_clear(rpt_ctx *c) {
    c->punctual_lights.release();
    c->punctual_lights_host.clear();
    c->punctual_share = 0.0f;
}

static bool finite3f(const float *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

/* Everything rpt_set_punctual_lights refuses that does not need a context: the setter and the host hooks (rpt_debug_punctual_lights_check, the two
 * rpt_debug_punctual_sample) share it, so the refusals can be held without a device.  mesh_lights: the scene's light table is not the sentinel. */
int rpt_punctual_lights_check(const rpt_punctual_light *lights, size_t n, float pick_share, bool mesh_lights, std::string &error) {
    const std::string who = "rpt_set_punctual_lights: ";
    if (!lights != (n == 0)) { error = who + "(NULL, 0) clears the lights; anything else needs both a buffer and a count"; return RPT_EINVAL; }
    if (n > 65535) { error = who + std::to_string(n) + " lights, at most 65535"; return RPT_EINVAL; }
    for (size_t i = 0; i < n; ++i) {
        const rpt_punctual_light &l = lights[i];
        const std::string rec = who + "record " + std::to_string(i);
        if (l.type > RPT_LIGHT_DIRECTIONAL) { error = rec + " has type " + std::to_string(l.type) + ", above RPT_LIGHT_DIRECTIONAL"; return RPT_EINVAL; }
        if (!finite3f(l.position) || !finite3f(l.direction) || !finite3f(l.intensity)) { error = rec + " has a position, direction or intensity that is not finite"; return RPT_EINVAL; }
        if (l.intensity[0] < 0.0f || l.intensity[1] < 0.0f || l.intensity[2] < 0.0f) { error = rec + " has a negative intensity"; return RPT_EINVAL; }
        if (l.type != RPT_LIGHT_POINT) {
            const double len2 = (double)l.direction[0] * l.direction[0] + (double)l.direction[1] * l.direction[1] + (double)l.direction[2] * l.direction[2];
            if (std::fabs(len2 - 1.0) > 1e-3) { error = rec + " has a direction that is not of unit length"; return RPT_EINVAL; }
        }
        if (!std::isfinite(l.angle_scale) || !std::isfinite(l.angle_offset)) { error = rec + " has an angle_scale or angle_offset that is not finite"; return RPT_EINVAL; }
        for (uint32_t r : l.reserved)
            if (r != 0u) { error = rec + " has a non-zero reserved word"; return RPT_EINVAL; }
    }
    if (n != 0 && mesh_lights && !(pick_share > 0.0f && pick_share < 1.0f)) {
        error = who + "pick_share must lie in (0, 1) while the scene has emissive triangles";
        return RPT_EINVAL;
    }
    return RPT_OK;
}

/* the device records of k_punctual.h: four float4 per light */
std::vector<float4> rpt_punctual_records(const rpt_punctual_light *lights, size_t n) {
    std::vector<float4> rec(4 * n);
    for (size_t i = 0; i < n; ++i) {
        const rpt_punctual_light &l = lights[i];
        rec[4 * i + 0] = make_float4(l.position[0], l.position[1], l.position[2], rptm::u2f(l.type));
        rec[4 * i + 1] = make_float4(l.direction[0], l.direction[1], l.direction[2], l.angle_scale);
        rec[4 * i + 2] = make_float4(l.intensity[0], l.intensity[1], l.intensity[2], l.angle_offset);
        rec[4 * i + 3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    return rec;
}

extern "C" {

int rpt_set_punctual_lights(rpt_ctx *c, const rpt_punctual_light *lights, size_t n, float pick_share) {
    if (!c) return RPT_EINVAL;
    if (!c->has_scene) { c->error = "rpt_set_punctual_lights: rpt_upload_scene must precede it"; return RPT_EINVAL; }
    const bool mesh_lights = c->scene.no_lights == 0u;
    std::string error;
    if (rpt_punctual_lights_check(lights, n, pick_share, mesh_lights, error) != RPT_OK) { c->error = error; return RPT_EINVAL; }
    /* nothing above touched the context; from here the batches enqueued so far finish with the lights they were enqueued with */
    RPT_TRY(rpt_wait(c));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!lights) { rpt_punctual_lights_clear(c); return RPT_OK; }
    /* the new records are built beside the old ones and take their place only once they are on the device: an allocation or a copy that fails leaves the
     * context with the lights, the records and the share it had */
    const std::vector<float4> rec = rpt_punctual_records(lights, n);
    DevBuf<float4> fresh;
    HIP_TRY(c, fresh.from_host(rec.data(), rec.size()));
    c->punctual_lights = std::move(fresh);
    c->punctual_lights_host.assign(lights, lights + n);
    c->punctual_share = mesh_lights ? pick_share : 1.0f;
    return RPT_OK;
}

int rpt_punctual_lights(rpt_ctx *c, rpt_punctual_light *out, size_t capacity, size_t *n_out, float *effective_share_out) {
    if (!c || !n_out) return RPT_EINVAL;
    *n_out = c->punctual_lights_host.size();
    if (effective_share_out) *effective_share_out = c->punctual_share;
    if (out) {
        if (capacity < c->punctual_lights_host.size()) { c->error = "rpt_punctual_lights: capacity below the light count"; return RPT_EINVAL; }
        if (!c->punctual_lights_host.empty()) memcpy(out, c->punctual_lights_host.data(), c->punctual_lights_host.size() * sizeof(rpt_punctual_light));
    }
    return RPT_OK;
}

int rpt_debug_punctual_lights_check(const rpt_punctual_light *lights, size_t n, float pick_share, int scene_has_emitters, char *message_out, size_t capacity) {
    std::string error;
    const int rc = rpt_punctual_lights_check(lights, n, pick_share, scene_has_emitters != 0, error);
    if (message_out && capacity) {
        const size_t k = error.size() < capacity - 1 ? error.size() : capacity - 1;
        memcpy(message_out, error.data(), k);
        message_out[k] = 0;
    }
    return rc;
}

int rpt_debug_force_punctual_kernels(rpt_ctx *c, int on) {
    if (!c) return RPT_EINVAL;
    c->force_punctual_kernels = on != 0;
    return RPT_OK;
}

}  // extern "C"
