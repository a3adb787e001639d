/*
 * lens_camera.h — the thin-lens camera ray of rpt_set_camera_lens (include/rpt/rpt.h) in the oracle's own vector types and math, written from the operation
 * order csrc/k_lens.h states in its comment, not through that header:
 *   j = gen_r2() (dimensions 1, 2),  uv as lib.rs:38-41,  uv *= tan_half_fov,  d = normalize(uv.x, uv.y, 1)
 *   aperture_radius == 0:  origin = cam_position,  direction = euler * d
 *   otherwise:             u1 = lds(n, 0, offset), u2 = lds(n, 31, offset) — the two table entries gen_r1 never reads for a path of at most 30 dimensions;
 *                          l = aperture_radius * sqrt(u1) * (cos, sin)(6.2831855f * u2),  pf = d * (focus_distance / d.z),
 *                          origin = cam_position + euler * (l.x, l.y, 0),  direction = euler * normalize(pf.x - l.x, pf.y - l.y, pf.z)
 * ONE text for the two restatements that start a path with it: tests/lens_oracle/lens_oracle.cpp (the reference's PBR surface) and
 * tests/models_oracle/models_oracle.cpp (a material's model at lib.rs:144).  Included AFTER oracle/rpt_oracle.cpp, whose internals it uses.
 */
#pragma once

namespace {

struct LensRecord { float tan_half_fov, aperture_radius, focus_distance; uint32_t reserved; };     /* rpt_camera_lens */

/* the camera ray of sample (rng.n, rng.offset) of pixel (id_x, id_y); rng_state has drawn the jitter when it returns (dimension 2) */
inline void lens_camera_ray(uint32_t id_x, uint32_t id_y, const rpt_tracing_config &config, const LensRecord &lens, RngState &rng_state, V3 &ray_origin, V3 &ray_direction) {
    V2 jitter = rng_state.gen_r2();
    V2 suv = V2{(float)id_x, (float)id_y} + jitter;
    V2 uv = V2{suv.x / (float)config.width, 1.0f - suv.y / (float)config.height} * 2.0f - V2{1.0f, 1.0f};
    uv.y *= (float)config.height / (float)config.width;
    uv = uv * lens.tan_half_fov;

    V3 d = normalize(v3(uv.x, uv.y, 1.0f));
    M3 euler_mat = mul(rotation_y(config.cam_rotation[1]), rotation_x(config.cam_rotation[0]));
    if (lens.aperture_radius == 0.0f) {
        ray_origin = xyz(config.cam_position);
        ray_direction = mul(euler_mat, d);
        return;
    }
    float u1 = lds(rng_state.n, 0u, rng_state.offset), u2 = lds(rng_state.n, 31u, rng_state.offset);
    float r = lens.aperture_radius * m_sqrt(u1);
    float phi = 6.2831855f * u2;
    float lx = r * m_cos(phi), ly = r * m_sin(phi);
    V3 pf = d * (lens.focus_distance / d.z);
    ray_origin = xyz(config.cam_position) + mul(euler_mat, v3(lx, ly, 0.0f));
    ray_direction = mul(euler_mat, normalize(v3(pf.x - lx, pf.y - ly, pf.z)));
}

/* a path that drew dimension 31 shares it with the lens sample (rpt_set_camera_lens refuses such a configuration): flagged like the reference's panic */
inline bool lens_shares_a_dimension(const LensRecord &lens, const RngState &rng_state) {
    return lens.aperture_radius != 0.0f && rng_state.dimension >= 31u;
}

}  // namespace
