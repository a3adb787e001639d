/*
 * k_punctual.h — punctual lights (include/rpt/rpt.h rpt_set_punctual_lights): the pick of one light among n and the term it sends to a surface point, the one
 * piece of arithmetic of the rule.  Called by the punctual variant of the surface stage (k_shade.h shade_slot<.., PUNCTUAL>, instantiated in rpt_punctual.hip
 * only) when the first light draw l1 falls below the effective share q, and, alone, by the test hooks rpt_debug_punctual_sample (device) and
 * rpt_debug_punctual_sample_host (the host build of this header).
 *
 * The device record, four float4 per light, built by the setter from rpt_punctual_light:
 *     [0] position x y z, type (the bits of RPT_LIGHT_*)     [1] direction x y z, angle_scale     [2] intensity r g b, angle_offset     [3] 0
 *
 * The f32 operations, in this order (every quotient an IEEE division, the root correctly rounded):
 *     j        = min(f2u32_sat((l1 / q) * (float)n), n - 1)
 *     pick_pdf = q / (float)n
 *   point, spot:
 *     v = P - hit      d = sqrt((v.x v.x + v.y v.y) + v.z v.z)      L = (v.x / d, v.y / d, v.z / d)      max_t = d - EPS * 2
 *     spot = 1, or for a spot light   a = min(max(((dir.x -L.x + dir.y -L.y) + dir.z -L.z) * angle_scale + angle_offset, 0), 1)   spot = a * a
 *     E = intensity * (spot / (d * d))
 *   directional:
 *     L = -dir      max_t = 1e6      E = intensity
 * A light at the hit point (d = 0) gives L = NaN and E = +inf (a spot light: NaN): the surface's diffuse pdf of a NaN direction is 0 (max(NaN, 0) = 0), so the
 * term is zero and nothing is queued.  min / max are Rust's: a NaN operand yields the other one.
 */
#ifndef RPT_K_PUNCTUAL_H
#define RPT_K_PUNCTUAL_H

#include "k_common.h"

#define RPT_PUNCTUAL_POINT 0u
#define RPT_PUNCTUAL_SPOT 1u
#define RPT_PUNCTUAL_DIRECTIONAL 2u
#define RPT_PUNCTUAL_EPS 0.001f          /* util.rs:5, the shadow ray's offsets (k_shade.h RPT_EPS) */
#define RPT_PUNCTUAL_FAR 1e6f            /* a directional light's max_t */

/* the kernel argument of the punctual variant: the records, their count and the effective share (0 with no lights) */
struct DevPunctual {
    const float4 *lights;
    uint32_t n;
    float q;
};

struct PunctualSample {
    uint32_t j;          /* the light picked */
    F3 L;                /* unit direction from the hit towards the light */
    float max_t;         /* of the shadow ray that leaves hit + L * EPS */
    F3 E;                /* what arrives, before the surface's own evaluate and the division by pick_pdf */
    float pick_pdf;
};

RPT_HD PunctualSample punctual_sample(F3 hit, float l1, const float4 *lights, uint32_t n, float q) {
    PunctualSample o;
    uint32_t j = rptm::f2u32_sat((l1 / q) * (float)n);
    if (j > n - 1u) j = n - 1u;
    o.j = j;
    o.pick_pdf = q / (float)n;
    const float4 r0 = lights[4u * j], r1 = lights[4u * j + 1u], r2 = lights[4u * j + 2u];
    const uint32_t type = rptm::f2u(r0.w);
    const F3 dir = f3(r1.x, r1.y, r1.z), intensity = f3(r2.x, r2.y, r2.z);
    if (type == RPT_PUNCTUAL_DIRECTIONAL) {
        o.L = -dir;
        o.max_t = RPT_PUNCTUAL_FAR;
        o.E = intensity;
    } else {
        const F3 v = f3(r0.x, r0.y, r0.z) - hit;
        const float d = rptm::sqrtr(dot3(v, v));
        o.L = v / d;
        o.max_t = d - RPT_PUNCTUAL_EPS * 2.0f;
        float spot = 1.0f;
        if (type == RPT_PUNCTUAL_SPOT) {
            const float a = rptm::fminr(rptm::fmaxr(dot3(dir, -o.L) * r1.w + r2.w, 0.0f), 1.0f);
            spot = a * a;
        }
        o.E = intensity * (spot / (d * d));
    }
    return o;
}

#endif /* RPT_K_PUNCTUAL_H */
