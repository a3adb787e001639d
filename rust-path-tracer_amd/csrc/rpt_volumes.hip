/*
 * rpt_volumes.hip — absorbing glass (include/rpt/rpt.h rpt_set_material_volumes): the absorption records beside the model records, and the volumes variant of
 * the surface stage, k_shade_volumes = the kernel text of k_shade (k_shade_body.h) with shade_slot<.., MODELS, VOLUMES>.  A translation unit of its own, and
 * the records one more argument of their own, as rpt_models.hip has it: no kernel of the other units changes for it.  dispatch_iteration (rpt_hip.hip)
 * launches this variant in place of k_shade_models when some Glass record carries a non-zero sigma (or the test hook asks), so every route into the pipeline
 * takes it; with no records, with every sigma zero or with no Glass material the launch is the one made without this unit.
 */
#include <cmath>
#include <cstring>

#include "rpt_ctx.h"

#include "k_shade.h"

static_assert(sizeof(rpt_material_volume) == sizeof(float4), "the kernels read a record as one float4: (sigma r, g, b, -)");

/* (no occupancy asked of the compiler, as for k_shade_models) */
#define RPT_SHADE_KERNEL k_shade_volumes
#define RPT_SHADE_MODELS true
#define RPT_SHADE_MODELS_ARG(...) __VA_ARGS__
#define RPT_SHADE_VOLUMES true
#define RPT_SHADE_VOLUMES_ARG(...) __VA_ARGS__
#define RPT_SHADE_PUNCTUAL false
#define RPT_SHADE_PUNCTUAL_ARG(...)
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
    if (c->shade_compact) k_shade_volumes<NEE, TEXTURED, true><<<(c->n_slots + RPT_BLOCK * RPT_SHADE_ROUNDS - 1) / (RPT_BLOCK * RPT_SHADE_ROUNDS), RPT_BLOCK, 0, c->stream>>>(c->scene, c->state, c->queues, c->cfg, iteration, c->dev_stats.p, c->call_samples, models, volumes);
    else k_shade_volumes<NEE, TEXTURED, false><<<blocks, RPT_BLOCK, 0, c->stream>>>(c->scene, c->state, c->queues, c->cfg, iteration, c->dev_stats.p, c->call_samples, models, volumes);
}

void rpt_launch_shade_volumes(rpt_ctx *c, uint32_t iteration, uint32_t blocks) {
    const bool tex = c->scene.textured != 0u;
    switch (c->cfg.nee_mode) {
        case RPT_NEE_MIS: return tex ? launch<RPT_NEE_MIS, true>(c, iteration, blocks) : launch<RPT_NEE_MIS, false>(c, iteration, blocks);
        case RPT_NEE_DIRECT: return tex ? launch<RPT_NEE_DIRECT, true>(c, iteration, blocks) : launch<RPT_NEE_DIRECT, false>(c, iteration, blocks);
        default: return tex ? launch<RPT_NEE_NONE, true>(c, iteration, blocks) : launch<RPT_NEE_NONE, false>(c, iteration, blocks);
    }
}

/* some Glass record has a volume record with a non-zero sigma: called by both setters and both clears, so the order of the two sets does not matter */
void rpt_material_volumes_recount(rpt_ctx *c) {
    bool in_use = false;
    if (c->material_volumes_host.size() == c->material_models_host.size())
        for (size_t i = 0; i < c->material_volumes_host.size(); ++i) {
            const rpt_material_volume &v = c->material_volumes_host[i];
            in_use = in_use || (c->material_models_host[i].model == RPT_MODEL_GLASS && (v.sigma[0] != 0.0f || v.sigma[1] != 0.0f || v.sigma[2] != 0.0f));
        }
    c->volumes_in_use = in_use;
}

/* rpt_upload_scene: the new scene's materials have no records */
void rpt_material_volumes_clear(rpt_ctx *c) {
    c->material_volumes.release();
    c->material_volumes_host.clear();
    c->volumes_in_use = false;
}

extern "C" {

int rpt_set_material_volumes(rpt_ctx *c, const rpt_material_volume *volumes, size_t n) {
    if (!c) return RPT_EINVAL;
    if (!c->has_scene) { c->error = "rpt_set_material_volumes: rpt_upload_scene must precede it"; return RPT_EINVAL; }
    if (!volumes != (n == 0)) { c->error = "rpt_set_material_volumes: (NULL, 0) clears the records; anything else needs both a buffer and a count"; return RPT_EINVAL; }
    if (volumes && n != c->n_materials) {
        c->error = "rpt_set_material_volumes: " + std::to_string(n) + " records for a scene of " + std::to_string(c->n_materials) + " materials";
        return RPT_EINVAL;
    }
    for (size_t i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k)
            if (!(std::isfinite(volumes[i].sigma[k]) && volumes[i].sigma[k] >= 0.0f)) {
                c->error = "rpt_set_material_volumes: sigma[" + std::to_string(k) + "] of record " + std::to_string(i) + " must be finite and not negative";
                return RPT_EINVAL;
            }
        if (volumes[i].reserved != 0u) { c->error = "rpt_set_material_volumes: record " + std::to_string(i) + " has a non-zero reserved word"; return RPT_EINVAL; }
    }
    /* nothing above touched the context; from here the batches enqueued so far finish with the records they were enqueued with */
    RPT_TRY(rpt_wait(c));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    /* (the denoiser's guides do not carry the transmittance: they stay valid) */
    if (!volumes) { rpt_material_volumes_clear(c); return RPT_OK; }
    if (c->material_volumes.n != n) HIP_TRY(c, c->material_volumes.alloc(n));
    HIP_TRY(c, hipMemcpy(c->material_volumes.p, volumes, n * sizeof(rpt_material_volume), hipMemcpyHostToDevice));
    c->material_volumes_host.assign(volumes, volumes + n);
    rpt_material_volumes_recount(c);
    return RPT_OK;
}

int rpt_material_volumes(rpt_ctx *c, rpt_material_volume *out, size_t capacity, size_t *n_out) {
    if (!c || !n_out) return RPT_EINVAL;
    *n_out = c->material_volumes_host.size();
    if (out) {
        if (capacity < c->material_volumes_host.size()) { c->error = "rpt_material_volumes: capacity below the record count"; return RPT_EINVAL; }
        if (!c->material_volumes_host.empty()) memcpy(out, c->material_volumes_host.data(), c->material_volumes_host.size() * sizeof(rpt_material_volume));
    }
    return RPT_OK;
}

int rpt_debug_force_volume_kernels(rpt_ctx *c, int on) {
    if (!c) return RPT_EINVAL;
    c->force_volume_kernels = on != 0;
    return RPT_OK;
}

int rpt_debug_last_shade_variant(rpt_ctx *c, uint32_t *variant_out) {
    if (!c || !variant_out) return RPT_EINVAL;
    *variant_out = c->last_shade_variant;
    return RPT_OK;
}

}  // extern "C"
