/*
 * k_lens.h — the thin-lens camera (include/rpt/rpt.h rpt_set_camera_lens): field of view, aperture and focus distance in place of the reference's pinhole
 * with its fixed 90 degree horizontal field of view (kernels/src/lib.rs:38-51, k_path.h camera_ray).  ONE RPT_HD function, lens_ray, is what the device
 * kernels (rpt_lens.hip: k_generate_lens, the lens builds of the completion kernels, k_lens_rays) and the host hook (rpt_debug_lens_rays_host) compile; it
 * uses only what rpt_math.h holds equal on both sides — sqrtr, sincosr, IEEE division, rcp_rn == 1.0f / x — and no contraction.
 *
 * The f32 operations, in this order (W, H, px, py converted to f32 first; P[i] = LDS_PRIMES[i], kernels/src/rng.rs:20-32; key = n + offset, wrapping;
 * u(i) = (f32)(P[i] * key mod 2^32) * 2^-32; cam = cam_position; E = DevConfig::euler, E * v = ((col0 * v.x) + (col1 * v.y)) + (col2 * v.z);
 * normalize(v) = v * (1 / sqrt((v.x v.x + v.y v.y) + v.z v.z))):
 *   1  j1 = u(1), j2 = u(2)                                   the reference's two jitter draws: the path goes on at dimension 2 as ever
 *      sx = px + j1, sy = py + j2
 *      ux = (sx / W) * 2 - 1
 *      uy = (1 - sy / H) * 2 - 1,  uy = uy * (H / W)
 *      ux = ux * tan_half_fov,  uy = uy * tan_half_fov           (a factor of 1.0f changes no bit)
 *      d = normalize(ux, uy, 1)
 *   2  aperture_radius == 0:  ro = cam,  rd = E * d             with tan_half_fov == 1 this is camera_ray bit for bit
 *   3  otherwise
 *      u1 = u(0), u2 = u(31)                                    the two entries of the table no path reads (gen_r1 increments before it reads; entry 31 only
 *                                                                by a configuration of 31 dimensions, which rpt_set_camera_lens / rpt_set_config refuse)
 *      r = aperture_radius * sqrt(u1)
 *      (s, c) = sincos(6.2831855f * u2),  lx = r * c,  ly = r * s
 *      k = focus_distance / d.z,  pf = d * k                    the point of the plane in focus that the pinhole ray meets (camera space)
 *      ro = cam + E * (lx, ly, 0)
 *      rd = E * normalize(pf.x - lx, pf.y - ly, pf.z)
 * lens_ray_centre is step 1 and 2 with (j1, j2) = (0.5, 0.5): the ray of the denoiser's guides, through the pixel centre and the LENS CENTRE — guides are
 * sharp on purpose, the aperture does not enter them.  tests/lens_oracle/lens_oracle.cpp restates this text; tests/test_camera_lens.py reads it in float64.
 */
#ifndef RPT_K_LENS_H
#define RPT_K_LENS_H

#include "k_common.h"

#define RPT_LENS_PRIME_J1 0xbb67ae84u      /* LDS_PRIMES[1], [2]: the jitter (k_common.h c_lds_primes, Rng::next from dimension 0) */
#define RPT_LENS_PRIME_J2 0x3c6ef372u
#define RPT_LENS_PRIME_U1 0x6a09e667u      /* LDS_PRIMES[0], [31]: the lens sample */
#define RPT_LENS_PRIME_U2 0x720dcdfcu
#define RPT_LENS_TWO_PI 6.2831855f         /* RN(2 pi) */

/* what the kernels take of an rpt_camera_lens (an argument of its own: DevConfig is what it was) */
struct DevLens {
    float tan_half_fov, aperture_radius, focus_distance;
};

RPT_HD float lens_unit(uint32_t prime, uint32_t key) { return (float)(prime * key) * (1.0f / 4294967296.0f); }
RPT_HD F3 lens_mat3_mul(const float *m, F3 v) {      /* k_path.h mat3_mul */
    F3 r = f3(m[0], m[1], m[2]) * v.x;
    r = r + (f3(m[3], m[4], m[5]) * v.y);
    r = r + (f3(m[6], m[7], m[8]) * v.z);
    return r;
}
RPT_HD F3 lens_norm3(F3 a) { return a * rptm::rcp_rn(rptm::sqrtr(dot3(a, a))); }      /* k_common.h norm3 */

/* step 1 from the jitter on: the unit direction through film point (px + j1, py + j2), camera space */
RPT_HD F3 lens_film_direction(const DevConfig &cfg, const DevLens &lens, uint32_t px, uint32_t py, float j1, float j2) {
    float sx = (float)px + j1, sy = (float)py + j2;
    float ux = (sx / (float)cfg.c.width) * 2.0f - 1.0f;
    float uy = (1.0f - sy / (float)cfg.c.height) * 2.0f - 1.0f;
    uy *= (float)cfg.c.height / (float)cfg.c.width;
    ux *= lens.tan_half_fov;
    uy *= lens.tan_half_fov;
    return lens_norm3(f3(ux, uy, 1.0f));
}

RPT_HD void lens_ray(const DevConfig &cfg, const DevLens &lens, uint32_t px, uint32_t py, uint32_t key, F3 &ro, F3 &rd) {
    const float j1 = lens_unit(RPT_LENS_PRIME_J1, key), j2 = lens_unit(RPT_LENS_PRIME_J2, key);
    const F3 d = lens_film_direction(cfg, lens, px, py, j1, j2);
    const F3 cam = f3(cfg.c.cam_position[0], cfg.c.cam_position[1], cfg.c.cam_position[2]);
    if (lens.aperture_radius == 0.0f) {
        ro = cam;
        rd = lens_mat3_mul(cfg.euler, d);
        return;
    }
    const float u1 = lens_unit(RPT_LENS_PRIME_U1, key), u2 = lens_unit(RPT_LENS_PRIME_U2, key);
    const float r = lens.aperture_radius * rptm::sqrtr(u1);
    float s, c;
    rptm::sincosr(RPT_LENS_TWO_PI * u2, s, c);
    const float lx = r * c, ly = r * s;
    const float k = lens.focus_distance / d.z;
    const F3 pf = d * k;
    ro = cam + lens_mat3_mul(cfg.euler, f3(lx, ly, 0.0f));
    rd = lens_mat3_mul(cfg.euler, lens_norm3(f3(pf.x - lx, pf.y - ly, pf.z)));
}

RPT_HD void lens_ray_centre(const DevConfig &cfg, const DevLens &lens, uint32_t px, uint32_t py, F3 &ro, F3 &rd) {
    ro = f3(cfg.c.cam_position[0], cfg.c.cam_position[1], cfg.c.cam_position[2]);
    rd = lens_mat3_mul(cfg.euler, lens_film_direction(cfg, lens, px, py, 0.5f, 0.5f));
}

#endif /* RPT_K_LENS_H */
