/*
 * rpt_models.hip — material models (include/rpt/rpt.h rpt_set_material_models): the records beside the material buffer, and the models variant of the
 * surface stage, k_shade_models = the kernel text of k_shade (k_shade_body.h) with shade_slot<.., MODELS>.  A translation unit of its own, and the records an argument of
 * their own: no kernel of the other units, and no struct one of them takes by value, changes for it.  dispatch_iteration (rpt_hip.hip) launches this
 * variant in place of k_shade when some record is not PBR (or the test hook asks), so every route into the pipeline takes it.
 */
#include <cmath>
#include <cstring>

#include "rpt_ctx.h"

#include "k_shade.h"

static_assert(sizeof(rpt_material_model) == sizeof(uint4), "the kernels read a record as one uint4: (model, ior bits, -, -)");
static_assert(RPT_MODEL_LAMBERTIAN == RPT_DEV_MODEL_LAMBERTIAN && RPT_MODEL_GLASS == RPT_DEV_MODEL_GLASS && RPT_MODEL_PBR == 0, "k_shade.h names the models by value");

/* (no occupancy asked of the compiler: the plain variants' 8 and 5 waves per SIMD would spill with three BSDFs in the body) */
#define RPT_SHADE_KERNEL k_shade_models
#define RPT_SHADE_MODELS true
#define RPT_SHADE_MODELS_ARG(...) __VA_ARGS__
#define RPT_SHADE_VOLUMES false
#define RPT_SHADE_VOLUMES_ARG(...)
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
    if (c->shade_compact) k_shade_models<NEE, TEXTURED, true><<<(c->n_slots + RPT_BLOCK * RPT_SHADE_ROUNDS - 1) / (RPT_BLOCK * RPT_SHADE_ROUNDS), RPT_BLOCK, 0, c->stream>>>(c->scene, c->state, c->queues, c->cfg, iteration, c->dev_stats.p, c->call_samples, models);
    else k_shade_models<NEE, TEXTURED, false><<<blocks, RPT_BLOCK, 0, c->stream>>>(c->scene, c->state, c->queues, c->cfg, iteration, c->dev_stats.p, c->call_samples, models);
}

void rpt_launch_shade_models(rpt_ctx *c, uint32_t iteration, uint32_t blocks) {
    const bool tex = c->scene.textured != 0u;
    switch (c->cfg.nee_mode) {
        case RPT_NEE_MIS: return tex ? launch<RPT_NEE_MIS, true>(c, iteration, blocks) : launch<RPT_NEE_MIS, false>(c, iteration, blocks);
        case RPT_NEE_DIRECT: return tex ? launch<RPT_NEE_DIRECT, true>(c, iteration, blocks) : launch<RPT_NEE_DIRECT, false>(c, iteration, blocks);
        default: return tex ? launch<RPT_NEE_NONE, true>(c, iteration, blocks) : launch<RPT_NEE_NONE, false>(c, iteration, blocks);
    }
}

/* rpt_upload_scene: the new scene's materials have no records */
void rpt_material_models_clear(rpt_ctx *c) {
    c->material_models.release();
    c->material_models_host.clear();
    c->models_in_use = false;
    rpt_material_volumes_recount(c);     /* (no Glass record: no volume record is in use) */
}

extern "C" {

int rpt_set_material_models(rpt_ctx *c, const rpt_material_model *models, size_t n_models) {
    if (!c) return RPT_EINVAL;
    if (!c->has_scene) { c->error = "rpt_set_material_models: rpt_upload_scene must precede it"; return RPT_EINVAL; }
    if (!models != (n_models == 0)) { c->error = "rpt_set_material_models: (NULL, 0) clears the records; anything else needs both a buffer and a count"; return RPT_EINVAL; }
    if (models && n_models != c->n_materials) {
        c->error = "rpt_set_material_models: " + std::to_string(n_models) + " records for a scene of " + std::to_string(c->n_materials) + " materials";
        return RPT_EINVAL;
    }
    bool in_use = false;
    for (size_t i = 0; i < n_models; ++i) {
        if (models[i].model > RPT_MODEL_GLASS) { c->error = "rpt_set_material_models: record " + std::to_string(i) + " has model " + std::to_string(models[i].model) + " (0 PBR, 1 Lambertian, 2 Glass)"; return RPT_EINVAL; }
        if (models[i].model == RPT_MODEL_GLASS && !(std::isfinite(models[i].ior) && models[i].ior > 0.0f)) {
            c->error = "rpt_set_material_models: the ior of Glass record " + std::to_string(i) + " must be finite and above 0";
            return RPT_EINVAL;
        }
        in_use = in_use || models[i].model != RPT_MODEL_PBR;
    }
    /* nothing above touched the context; from here the batches enqueued so far finish with the records they were enqueued with */
    RPT_TRY(rpt_wait(c));
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->dn.through_glass != 0u) c->dn.guides_valid = false;       /* rpt_set_guides_through_glass: the guides follow the Glass records */
    if (!models) { rpt_material_models_clear(c); return RPT_OK; }
    if (c->material_models.n != n_models) HIP_TRY(c, c->material_models.alloc(n_models));
    HIP_TRY(c, hipMemcpy(c->material_models.p, models, n_models * sizeof(rpt_material_model), hipMemcpyHostToDevice));
    c->material_models_host.assign(models, models + n_models);
    c->models_in_use = in_use;
    rpt_material_volumes_recount(c);     /* (rpt_set_material_volumes: a volume record counts on a Glass material only) */
    return RPT_OK;
}

int rpt_material_models(rpt_ctx *c, rpt_material_model *out, size_t capacity, size_t *n_out) {
    if (!c || !n_out) return RPT_EINVAL;
    *n_out = c->material_models_host.size();
    if (out) {
        if (capacity < c->material_models_host.size()) { c->error = "rpt_material_models: capacity below the record count"; return RPT_EINVAL; }
        if (!c->material_models_host.empty()) memcpy(out, c->material_models_host.data(), c->material_models_host.size() * sizeof(rpt_material_model));
    }
    return RPT_OK;
}

int rpt_debug_force_model_kernels(rpt_ctx *c, int on) {
    if (!c) return RPT_EINVAL;
    c->force_model_kernels = on != 0;
    return RPT_OK;
}

}  // extern "C"
