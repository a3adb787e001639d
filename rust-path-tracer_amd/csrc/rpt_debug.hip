/*
 * rpt_debug.hip — the test hooks of include/rpt/rpt_debug.h that run kernels of their own: the math functions, the BSDF
 * pieces, the image sampler and single rays through the debug and the production traversal stages.
 */
#include <algorithm>
#include <cstring>

#include "rpt_ctx.h"
#include "rpt_fastdiv.h"
#include "k_gather.h"
#include "k_shade.h"             /* sample_by_lod: the function the shade stage, the sky stage and the denoiser's guides inline (k_shade itself is not instantiated); k_bsdf_extra.h */

/* one coordinate per thread through the production sampler, on an image of the hook's own */
template <bool IS_U8>
__global__ __launch_bounds__(256) void k_debug_sample_image(DevImage img, size_t n, const float2 *coords, float4 *out) {
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    out[i] = sample_by_lod<IS_U8>(img, coords[i].x, coords[i].y);
}

/* rpt_debug_bsdf: the functions of k_bsdf_extra.h, one item per thread (see oracle_bsdf for the item layout) */
__global__ void k_debug_bsdf(int kind, size_t n, const float *in, float *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 16 * i;
    F3 view = f3(p[0], p[1], p[2]), normal = f3(p[3], p[4], p[5]), r = f3(p[6], p[7], p[8]), albedo = f3(p[9], p[10], p[11]);
    BsdfSample o;
    o.pdf = 0.0f; o.lobe = 0u; o.spectrum = f3s(0.0f); o.direction = f3s(0.0f);
    if (kind == 0) o = lambertian_sample(albedo, normal, r);
    else if (kind == 1) o = glass_sample(albedo, p[12], p[13], view, normal, r);
    else if (kind == 2) lambertian_evaluate(albedo, normal, r, o.spectrum, o.pdf);
    else { o.lobe = rptm::f2u32_sat(r.x); o.spectrum = o.lobe == 1u ? f3s(1.0f) : albedo; o.pdf = 1.0f; }   /* bsdf.rs:115-128, 170-176 */
    float *q = out + 8 * i;
    q[0] = o.pdf; q[1] = __uint_as_float(o.lobe);
    q[2] = o.spectrum.x; q[3] = o.spectrum.y; q[4] = o.spectrum.z;
    q[5] = o.direction.x; q[6] = o.direction.y; q[7] = o.direction.z;
}

extern "C" {

/* ops 20 .. 31: the DOUBLE a building block of rpt_math.h returns, before the rounding to float hides all but a 2^-29th of it: a device Horner step
 * with two roundings instead of the fma changes no float of a million samples, and every one of these words.  Outside a block's domain: 0. */
RPT_HD double debug_math_core(int k, float x) {
    const double d = (double)x;
    const bool unit = x >= -1.0f && x <= 1.0f;
    switch (k) {
        case 0: return unit ? rptm::sin_poly(d) : 0.0;
        case 1: return unit ? rptm::cos_poly(d) : 0.0;
        case 2: return (x >= -700.0f && x <= 700.0f) ? rptm::exp_core(d) : 0.0;
        case 3: return (x > 0.0f && rptm::finiter(x)) ? rptm::log_core(d) : 0.0;
        case 4: return unit ? rptm::asin_poly(d, d * d) : 0.0;
        default: return (x >= 0.0f && x <= 1.0f) ? rptm::atan01(d) : 0.0;
    }
}

/* the operations of the math hooks: one statement for the kernel and for the host build of rpt_math.h (clang's, as tests/test_math.py needs) */
RPT_HD float debug_math_op(int op, float x, float y) {
    if (op >= 20) {
        const uint64_t u = rptm::d2u(debug_math_core((op - 20) >> 1, x));
        return rptm::u2f((uint32_t)((op & 1) ? u >> 32 : u));
    }
    switch (op) {
        case 0: return rptm::sinr(x);
        case 1: return rptm::cosr(x);
        case 2: return rptm::acosr(x);
        case 3: return rptm::expr(x);
        case 4: return rptm::powr(x, y);
        case 5: return rptm::asinr(x);
        case 6: return rptm::atan2r(x, y);
        case 7: return rptm::sqrtr(x);
        case 9: return rptm::slab_quotient(x, 0.0f, y);
        case 10: return rptm::exp_sky(x);
        case 11: return rptm::unorm8(x);
        case 12: return rptm::fminr(x, y);
        case 13: return rptm::fmaxr(x, y);
        case 14: return rptm::floorr(x);
        case 15: return rptm::ceilr(x);
        case 16: return rptm::u2f(rptm::f2u32_sat(x));      /* the word's bits */
        case 17: return rptm::atanr(x);
        case 18: return rptm::powi5(x);
        case 19: return rptm::absr(x);
        default: return x / y;
    }
}

__global__ void k_debug_math(int op, const float *x, const float *y, float *out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = debug_math_op(op, x[i], y[i]);
}

int rpt_debug_math_host(int op, const float *x, const float *y, float *out, size_t n) {
    if (op < 0 || op > 31 || !x || !y || !out) return RPT_EINVAL;
    for (size_t i = 0; i < n; ++i) out[i] = debug_math_op(op, x[i], y[i]);
    return RPT_OK;
}

int rpt_debug_math(rpt_ctx *c, int op, const float *x, const float *y, float *out, size_t n) {
    if (!c || op < 0 || op > 31 || !x || !y || !out) return RPT_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float> dx, dy, dout;
    HIP_TRY(c, dx.from_host(x, n)); HIP_TRY(c, dy.from_host(y, n)); HIP_TRY(c, dout.alloc(n));
    k_debug_math<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(op, dx.p, dy.p, dout.p, n);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}

/* Exhaustive check of a cheap exact operation against its IEEE form, over the bit patterns [lo_bits, lo_bits + count):
 * op 0: rptm::sqrtr == the compiler's correctly rounded sqrtf (trivially, today: the hook experiments with cheaper roots used); op 1: rptm::div_const_nontiny(x, y, RN(1 / y)) == x / y;
 * op 2: rptm::f2i32_sat (one v_cvt_i32_f32) == Rust's `f32 as i32` written out with its branches (results compared as bit patterns). */
__global__ void k_debug_math_sweep(int op, uint32_t lo_bits, unsigned long long count, float y, float ry, unsigned long long *out) {
    unsigned long long bad = 0ull;
    uint32_t first = 0xffffffffu;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t bits = lo_bits + (uint32_t)i;
        const float x = rptm::u2f(bits);
        const float fast = op == 0 ? rptm::sqrtr(x) : (op == 1 ? rptm::div_const_nontiny(x, y, ry) : rptm::u2f((uint32_t)rptm::f2i32_sat(x)));
        const float ieee = op == 0 ? __builtin_sqrtf(x) : (op == 1 ? x / y : rptm::u2f((uint32_t)rptm::f2i32_sat_reference(x)));
        const bool same = rptm::f2u(fast) == rptm::f2u(ieee) || (op != 2 && fast != fast && ieee != ieee);     /* (op 2 carries integers: bit patterns only) */
        if (!same) { bad += 1ull; first = first < bits ? first : bits; }
    }
    if (bad != 0ull) {
        atomicAdd(&out[0], bad);
        atomicMin(&out[1], (unsigned long long)first);
    }
}

int rpt_debug_math_sweep(rpt_ctx *c, int op, uint32_t lo_bits, uint64_t count, float y, uint64_t *mismatches_out, uint32_t *first_bad_bits_out) {
    if (!c || op < 0 || op > 2 || !mismatches_out || count > 0x100000000ull) return RPT_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<unsigned long long> d;
    HIP_TRY(c, d.alloc(2));
    unsigned long long h[2] = {0ull, 0xffffffffull};
    HIP_TRY(c, hipMemcpy(d.p, h, sizeof(h), hipMemcpyHostToDevice));
    k_debug_math_sweep<<<4096, 256, 0, c->stream>>>(op, lo_bits, (unsigned long long)count, y, 1.0f / y, d.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(h, d.p, sizeof(h), hipMemcpyDeviceToHost));
    *mismatches_out = h[0];
    if (first_bad_bits_out) *first_bad_bits_out = (uint32_t)h[1];
    return RPT_OK;
}

/* rptm::rcp_rn (rpt_rcp.h) against the compiler's `1.0f / x`, word for word (no NaN == NaN: the fallback IS that division; window != 0: rcp_rn_window), over the bit patterns
 * [lo_bits, lo_bits + count): out[0] the differences, out[1] how many of them out[2 ..] lists (any 64 of them: whichever threads came first) */
__global__ void k_debug_rcp_sweep(int window, uint32_t lo_bits, unsigned long long count, unsigned long long *out) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t bits = lo_bits + (uint32_t)i;
        const float x = rptm::u2f(bits);
        if (rptm::f2u(window ? rptm::rcp_rn_window(x) : rptm::rcp_rn(x)) != rptm::f2u(1.0f / x)) {
            atomicAdd(&out[0], 1ull);
            const unsigned long long k = atomicAdd(&out[1], 1ull);
            if (k < 64ull) out[2 + k] = bits;
        }
    }
}

int rpt_debug_rcp_sweep(rpt_ctx *c, int window, uint32_t lo_bits, uint64_t count, uint64_t *mismatches_out, uint32_t *bad_bits_out /* [64] */) {
    if (!c || !mismatches_out || !bad_bits_out || count > 0x100000000ull) return RPT_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<unsigned long long> d;
    HIP_TRY(c, d.alloc(66));
    unsigned long long h[66] = {};
    HIP_TRY(c, hipMemcpy(d.p, h, sizeof(h), hipMemcpyHostToDevice));
    k_debug_rcp_sweep<<<4096, 256, 0, c->stream>>>(window, lo_bits, (unsigned long long)count, d.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(h, d.p, sizeof(h), hipMemcpyDeviceToHost));
    *mismatches_out = h[0];
    for (int k = 0; k < 64; ++k) bad_bits_out[k] = (uint64_t)k < h[0] ? (uint32_t)h[2 + k] : 0xffffffffu;
    return RPT_OK;
}

__global__ void k_debug_rcp(int window, const float *x, float *out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = window ? rptm::rcp_rn_window(x[i]) : rptm::rcp_rn(x[i]);
}

int rpt_debug_rcp(rpt_ctx *c, int window, const float *x, float *out, size_t n) {
    if (!c || !x || !out) return RPT_EINVAL;
    if (n == 0) return RPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float> dx, dout;
    HIP_TRY(c, dx.from_host(x, n)); HIP_TRY(c, dout.alloc(n));
    k_debug_rcp<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(window, dx.p, dout.p, n);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, dout.p, n * 4, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_debug_bsdf(rpt_ctx *c, int kind, size_t n, const float *in, float *out) {
    if (!c || kind < 0 || kind > 3 || !in || !out) return RPT_EINVAL;
    if (n == 0) return RPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float> din, dout;
    HIP_TRY(c, din.from_host(in, 16 * n)); HIP_TRY(c, dout.alloc(8 * n));
    k_debug_bsdf<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(kind, n, din.p, dout.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, dout.p, 32 * n, hipMemcpyDeviceToHost));
    return RPT_OK;
}

__global__ void k_debug_volume_transmit(const float *thr, const float *sigma, const float *t, size_t n, float *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const F3 o = vol_transmit(f3(thr[3 * i], thr[3 * i + 1], thr[3 * i + 2]), f3(sigma[3 * i], sigma[3 * i + 1], sigma[3 * i + 2]), t[i]);
    out[3 * i] = o.x; out[3 * i + 1] = o.y; out[3 * i + 2] = o.z;
}

int rpt_debug_volume_transmit(rpt_ctx *c, int on_device, const float *thr, const float *sigma, const float *t, size_t n, float *out) {
    if (!thr || !sigma || !t || !out || (on_device && !c)) return RPT_EINVAL;
    if (n == 0) return RPT_OK;
    if (!on_device) {
        for (size_t i = 0; i < n; ++i) {
            const F3 o = vol_transmit(f3(thr[3 * i], thr[3 * i + 1], thr[3 * i + 2]), f3(sigma[3 * i], sigma[3 * i + 1], sigma[3 * i + 2]), t[i]);
            out[3 * i] = o.x; out[3 * i + 1] = o.y; out[3 * i + 2] = o.z;
        }
        return RPT_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float> dthr, dsigma, dt, dout;
    HIP_TRY(c, dthr.from_host(thr, 3 * n)); HIP_TRY(c, dsigma.from_host(sigma, 3 * n)); HIP_TRY(c, dt.from_host(t, n)); HIP_TRY(c, dout.alloc(3 * n));
    k_debug_volume_transmit<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(dthr.p, dsigma.p, dt.p, n, dout.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out, dout.p, 12 * n, hipMemcpyDeviceToHost));
    return RPT_OK;
}

/* the records a hook may sample: what the setter accepts, with any share in (0, 1] */
static bool punctual_hook_refuses(const rpt_punctual_light *lights, size_t n_lights, float q) {
    std::string error;
    return !lights || n_lights == 0 || !(q > 0.0f && q <= 1.0f) || rpt_punctual_lights_check(lights, n_lights, 0.5f, false, error) != RPT_OK;
}

RPT_HD void punctual_item(const float4 *lights, uint32_t n_lights, float q, const float *hits, const float *l1, size_t i, uint32_t *j_out, float *dirs, float *max_t,
                          float *e_out, float *pick_pdf) {
    const PunctualSample o = punctual_sample(f3(hits[3 * i], hits[3 * i + 1], hits[3 * i + 2]), l1[i], lights, n_lights, q);
    j_out[i] = o.j;
    dirs[3 * i] = o.L.x; dirs[3 * i + 1] = o.L.y; dirs[3 * i + 2] = o.L.z;
    max_t[i] = o.max_t;
    e_out[3 * i] = o.E.x; e_out[3 * i + 1] = o.E.y; e_out[3 * i + 2] = o.E.z;
    pick_pdf[i] = o.pick_pdf;
}

__global__ void k_debug_punctual_sample(const float4 *lights, uint32_t n_lights, float q, const float *hits, const float *l1, size_t n, uint32_t *j_out, float *dirs,
                                        float *max_t, float *e_out, float *pick_pdf) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    punctual_item(lights, n_lights, q, hits, l1, i, j_out, dirs, max_t, e_out, pick_pdf);
}

int rpt_debug_punctual_sample_host(const rpt_punctual_light *lights, size_t n_lights, float q, const float *hits, const float *l1, size_t n, uint32_t *j_out,
                                   float *dirs, float *max_t, float *e_out, float *pick_pdf) {
    if (punctual_hook_refuses(lights, n_lights, q) || !hits || !l1 || !j_out || !dirs || !max_t || !e_out || !pick_pdf) return RPT_EINVAL;
    const std::vector<float4> rec = rpt_punctual_records(lights, n_lights);
    for (size_t i = 0; i < n; ++i) punctual_item(rec.data(), (uint32_t)n_lights, q, hits, l1, i, j_out, dirs, max_t, e_out, pick_pdf);
    return RPT_OK;
}

int rpt_debug_punctual_sample(rpt_ctx *c, const rpt_punctual_light *lights, size_t n_lights, float q, const float *hits, const float *l1, size_t n, uint32_t *j_out,
                              float *dirs, float *max_t, float *e_out, float *pick_pdf) {
    if (!c || punctual_hook_refuses(lights, n_lights, q) || !hits || !l1 || !j_out || !dirs || !max_t || !e_out || !pick_pdf) return RPT_EINVAL;
    if (n == 0) return RPT_OK;
    const std::vector<float4> rec = rpt_punctual_records(lights, n_lights);
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float4> drec;
    DevBuf<float> dhits, dl1, ddirs, dmax_t, de, dpdf;
    DevBuf<uint32_t> dj;
    HIP_TRY(c, drec.from_host(rec.data(), rec.size())); HIP_TRY(c, dhits.from_host(hits, 3 * n)); HIP_TRY(c, dl1.from_host(l1, n));
    HIP_TRY(c, dj.alloc(n)); HIP_TRY(c, ddirs.alloc(3 * n)); HIP_TRY(c, dmax_t.alloc(n)); HIP_TRY(c, de.alloc(3 * n)); HIP_TRY(c, dpdf.alloc(n));
    k_debug_punctual_sample<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(drec.p, (uint32_t)n_lights, q, dhits.p, dl1.p, n, dj.p, ddirs.p, dmax_t.p, de.p, dpdf.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(j_out, dj.p, 4 * n, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(dirs, ddirs.p, 12 * n, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(max_t, dmax_t.p, 4 * n, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(e_out, de.p, 12 * n, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(pick_pdf, dpdf.p, 4 * n, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_debug_sample_image(rpt_ctx *c, int is_u8, const void *texels, uint32_t width, uint32_t height, size_t n, const float *coords_uv, float *out_rgba) {
    if (!c || !texels || !coords_uv || !out_rgba || width == 0u || height == 0u) return RPT_EINVAL;
    /* the limits of rpt_upload_scene: texel indices are 32-bit in sample_by_lod */
    if ((uint64_t)width * height > (is_u8 ? (1ull << 30) : (1ull << 28)) || n > 0xffffffffull) return RPT_EINVAL;
    if (n == 0) return RPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_texels = (size_t)width * height;
    DevBuf<uchar4> d_u8;
    DevBuf<float4> d_f32, d_out;
    DevBuf<float2> d_uv;
    if (is_u8) HIP_TRY(c, d_u8.from_host(static_cast<const uchar4 *>(texels), n_texels));
    else HIP_TRY(c, d_f32.from_host(static_cast<const float4 *>(texels), n_texels));
    HIP_TRY(c, d_uv.from_host(reinterpret_cast<const float2 *>(coords_uv), n)); HIP_TRY(c, d_out.alloc(n));
    const unsigned blocks = (unsigned)((n + 255) / 256);
    if (is_u8) k_debug_sample_image<true><<<blocks, 256, 0, c->stream>>>(DevImage{d_u8.p, width, height}, n, d_uv.p, d_out.p);
    else k_debug_sample_image<false><<<blocks, 256, 0, c->stream>>>(DevImage{d_f32.p, width, height}, n, d_uv.p, d_out.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out_rgba, d_out.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_debug_trace_rays(rpt_ctx *c, int any_hit, size_t n, const float *origins, const float *dirs, const float *max_t,
                         float *out_t, uint32_t *out_tri, uint32_t *out_flags) {
    if (!c || !origins || !dirs || !out_t || !out_tri || !out_flags || (any_hit && !max_t)) return RPT_EINVAL;
    if (!c->has_scene) { c->error = "no scene"; return RPT_EINVAL; }
    if (n == 0) return RPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float> d_o, d_d, d_m, d_t;
    DevBuf<uint32_t> d_tri, d_fl;
    HIP_TRY(c, d_o.from_host(origins, 3 * n)); HIP_TRY(c, d_d.from_host(dirs, 3 * n)); HIP_TRY(c, d_t.alloc(n));
    HIP_TRY(c, d_tri.alloc(n)); HIP_TRY(c, d_fl.alloc(n));
    HIP_TRY(c, max_t ? d_m.from_host(max_t, n) : d_m.alloc(n));
    rpt_launch_trace_debug(c, any_hit, (uint32_t)n, d_o.p, d_d.p, d_m.p, d_t.p, d_tri.p, d_fl.p);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(out_t, d_t.p, 4 * n, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(out_tri, d_tri.p, 4 * n, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(out_flags, d_fl.p, 4 * n, hipMemcpyDeviceToHost));
    return RPT_OK;
}

/* The same question through the PRODUCTION stages (rpt_debug_walk_production; rpt_debug_trace_rays_production is its NEAREST_PLAIN kind).  The nearest kinds:
 * the rays are written into the context's own slots as pending extension rays — as k_generate_first leaves a slot: HIT_PENDING —, the traversal stage is
 * launched exactly as an iteration of rpt_render launches it for this scene and state (rpt_launch_nearest: persistent LDS stream, PLAIN / FIRST / LAST;
 * streamed global-memory walk with or without cooperative leaves; the generic walk — per scene and developer knobs), and the hit records it wrote are read
 * back.  LAST runs in the form that writes hit records (implicit_zero == 0); its path-ending form — emission added, misses parked, HIT_DONE written by the
 * walk — and FIRST starting its own paths are covered by renders only.  Needs a configuration (the slots); leaves the context as after rpt_reset with
 * nothing rendered — call rpt_reset before rendering again. */
__global__ __launch_bounds__(RPT_BLOCK) void k_debug_load_rays(DevState st, uint32_t n, const float *origins, const float *dirs) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    st.ray_a[i] = make_float4(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], dirs[3 * i]);
    st.ray_b[i] = make_float2(dirs[3 * i + 1], dirs[3 * i + 2]);
    set_hit_word(st, i, HIT_PENDING);
}

/* The SHADOW kind of rpt_debug_walk_production: ray i becomes entry i - first[s] of shard s, first[s] <= i < first[s + 1], of the sharded shadow queue
 * (k_common.h q_position) with the tag "slot i, the path goes on" and the contribution (1, 1 + i % 4093, 0); the slot's radiance record and the streamed
 * walk's entry counter are zeroed and the shard counters set, as the shade stage that fills the queue in a render leaves them (Q_DRAINED stays 0). */
struct DebugShards { uint32_t first[RPT_Q_SHARDS + 1]; };
__global__ __launch_bounds__(RPT_BLOCK) void k_debug_load_shadow(DevState st, DevQueues q, uint32_t n, DebugShards sh, const float *origins, const float *dirs, const float *max_t) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i < RPT_Q_SHARDS) q.shadow_cnt[i * RPT_Q_SHARD_STRIDE] = sh.first[i + 1] - sh.first[i];
    if (i == 0u) q.count[Q_SPOOL] = 0u;
    if (i >= n) return;
    uint32_t s = 0u;
    while (i >= sh.first[s + 1]) s += 1u;
    const uint32_t at = q_position(s, i - sh.first[s]);
    q.sh_o[at] = make_float4(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], max_t[i]);
    q.sh_d[at] = make_float4(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], __uint_as_float(i));
    q.sh_c[at] = make_float4(1.0f, (float)(1u + i % 4093u), 0.0f, 0.0f);
    st.rad[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

/* the shares of the shards: shard s takes 1 + (7 s + 3) % 16 parts of 136 (a permutation of 1 .. 16, the largest share in shard 4, the smallest in shard 11),
 * what is left over goes to shard 4 too — one ray alone sits at position 1 024, behind four chunks of unfilled positions */
static DebugShards debug_shadow_shards(uint32_t n, uint32_t &most) {
    DebugShards sh;
    uint32_t cnt[RPT_Q_SHARDS], given = 0u;
    for (uint32_t s = 0; s < RPT_Q_SHARDS; ++s) { cnt[s] = (uint32_t)((uint64_t)n * (1u + (7u * s + 3u) % 16u) / 136u); given += cnt[s]; }
    cnt[4] += n - given;
    most = 0u;
    sh.first[0] = 0u;
    for (uint32_t s = 0; s < RPT_Q_SHARDS; ++s) { sh.first[s + 1] = sh.first[s] + cnt[s]; most = std::max(most, cnt[s]); }
    return sh;
}

static int debug_walk_shadow(rpt_ctx *c, size_t n, const float *origins, const float *dirs, const float *max_t, uint32_t *out_flags) {
    uint32_t most = 0u;
    const DebugShards sh = debug_shadow_shards((uint32_t)n, most);
    /* the positions the consumers sweep (k_common.h q_extent) must lie inside the queue arrays AND inside the grids rpt_launch_shadow sizes by the slot count */
    const uint64_t positions = (uint64_t)((most + 255u) >> 8) * (256u * RPT_Q_SHARDS);
    if (positions > (uint64_t)c->n_slots + RPT_Q_SLACK) {
        c->error = "rpt_debug_walk_production: " + std::to_string(n) + " shadow rays, filled unevenly, span " + std::to_string(positions) + " queue positions; the queue of this configuration has " +
                   std::to_string((uint64_t)c->n_slots + RPT_Q_SLACK);
        return RPT_EINVAL;
    }
    RPT_TRY(ensure_slot_state(c, c->n_slots, true, false));
    DevBuf<float> d_o, d_d, d_m;
    HIP_TRY(c, d_o.from_host(origins, 3 * n)); HIP_TRY(c, d_d.from_host(dirs, 3 * n)); HIP_TRY(c, d_m.from_host(max_t, n));
    hipStream_t s = c->stream;
    RPT_TRY(rpt_idle_all_slots(c));
    k_debug_load_shadow<<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(c->state, c->queues, (uint32_t)n, sh, d_o.p, d_d.p, d_m.p);
    rpt_launch_shadow(c);
    std::vector<float4> rad(n);
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpy(rad.data(), c->rad.p, n * sizeof(float4), hipMemcpyDeviceToHost));
    RPT_TRY(rpt_idle_all_slots(c));             /* back to "nothing in flight": the shard counters too */
    HIP_TRY(c, hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i) {
        const float4 r = rad[i];
        const bool occluded = r.x == 0.0f && r.y == 0.0f && r.z == 0.0f, visible = r.x == 1.0f && r.y == (float)(1u + (uint32_t)i % 4093u) && r.z == 0.0f;
        if (!occluded && !visible) {
            c->error = "rpt_debug_walk_production: shadow ray " + std::to_string(i) + " left the radiance (" + std::to_string(r.x) + ", " + std::to_string(r.y) + ", " + std::to_string(r.z) +
                       ") in its slot: neither nothing nor its own contribution";
            return RPT_EHIP;
        }
        out_flags[i] = occluded ? 1u : 0u;
    }
    return RPT_OK;
}

/* the nearest kinds: `who` names the entry point in the messages */
static int debug_walk_nearest(rpt_ctx *c, const char *who, int kind, size_t n, const float *origins, const float *dirs, float *out_t, uint32_t *out_tri, uint32_t *out_flags) {
    RPT_TRY(ensure_slot_state(c, c->n_slots, false, false));
    DevBuf<float> d_o, d_d;
    HIP_TRY(c, d_o.from_host(origins, 3 * n)); HIP_TRY(c, d_d.from_host(dirs, 3 * n));
    hipStream_t s = c->stream;
    RPT_TRY(rpt_idle_all_slots(c));
    k_debug_load_rays<<<rpt_blocks(n), RPT_BLOCK, 0, s>>>(c->state, (uint32_t)n, d_o.p, d_d.p);
    if (kind == RPT_WALK_NEAREST_LAST) {
        /* the form that writes hit records (k_traverse_nearest.h: done_here false), whatever the last render call left in the flag */
        const uint32_t implicit_zero = c->queues.implicit_zero;
        c->queues.implicit_zero = 0u;
        rpt_launch_nearest(c, 0u, true, false, false);
        c->queues.implicit_zero = implicit_zero;
    } else {
        rpt_launch_nearest(c, 0u, false, kind == RPT_WALK_NEAREST_FIRST, false);
    }
    std::vector<float2> hits(n);
    HIP_TRY(c, hipStreamSynchronize(s));
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpy(hits.data(), c->hit.p, n * sizeof(float2), hipMemcpyDeviceToHost));
    RPT_TRY(rpt_idle_all_slots(c));             /* back to "nothing in flight" */
    HIP_TRY(c, hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i) {
        uint32_t w;
        memcpy(&w, &hits[i].y, 4);
        if (w == HIT_PENDING || w == HIT_IDLE) { c->error = std::string(who) + ": ray " + std::to_string(i) + " was not traversed"; return RPT_EHIP; }
        out_t[i] = hits[i].x;
        out_tri[i] = (w == HIT_MISS) ? 0u : (w & 0x7fffffffu);
        out_flags[i] = (w == HIT_MISS) ? 0u : (1u | ((w >> 31) << 1));
    }
    return RPT_OK;
}

static int debug_walk_production(rpt_ctx *c, const char *who, int kind, size_t n, const float *origins, const float *dirs, const float *max_t, float *out_t, uint32_t *out_tri,
                                 uint32_t *out_flags) {
    if (!c) return RPT_EINVAL;
    if (kind < RPT_WALK_NEAREST_PLAIN || kind > RPT_WALK_SHADOW) { c->error = std::string(who) + ": no such kind of walk"; return RPT_EINVAL; }
    if (!origins || !dirs || !out_t || !out_tri || !out_flags) { c->error = std::string(who) + ": null ray or result arrays"; return RPT_EINVAL; }
    if (kind == RPT_WALK_SHADOW && !max_t) { c->error = std::string(who) + ": shadow rays need max_t"; return RPT_EINVAL; }
    if (!c->has_scene || !c->has_state) { c->error = std::string(who) + ": needs a scene and a configuration"; return RPT_EINVAL; }
    if (n == 0) return RPT_OK;
    if (n > c->n_slots) { c->error = std::string(who) + ": more rays than the context has slots (" + std::to_string(c->n_slots) + ")"; return RPT_EINVAL; }
    if (kind == RPT_WALK_NEAREST_FIRST) {
        for (size_t i = 0; i < n; ++i)
            if (memcmp(origins + 3 * i, c->cfg.c.cam_position, 3 * sizeof(float)) != 0) {
                c->error = std::string(who) + ": the origin of ray " + std::to_string(i) + " is not the configuration's cam_position, which the FIRST walk subtracts from its planes";
                return RPT_EINVAL;
            }
    }
    RPT_TRY(rpt_wait(c));
    HIP_TRY(c, hipSetDevice(c->device));
    if (kind == RPT_WALK_SHADOW) {
        memset(out_t, 0, n * sizeof(float)); memset(out_tri, 0, n * sizeof(uint32_t));
        return debug_walk_shadow(c, n, origins, dirs, max_t, out_flags);
    }
    return debug_walk_nearest(c, who, kind, n, origins, dirs, out_t, out_tri, out_flags);
}

int rpt_debug_trace_rays_production(rpt_ctx *c, size_t n, const float *origins, const float *dirs, float *out_t, uint32_t *out_tri, uint32_t *out_flags) {
    return debug_walk_production(c, "rpt_debug_trace_rays_production", RPT_WALK_NEAREST_PLAIN, n, origins, dirs, nullptr, out_t, out_tri, out_flags);
}

int rpt_debug_walk_production(rpt_ctx *c, int kind, size_t n, const float *origins, const float *dirs, const float *max_t, float *out_t, uint32_t *out_tri, uint32_t *out_flags) {
    return debug_walk_production(c, "rpt_debug_walk_production", kind, n, origins, dirs, max_t, out_t, out_tri, out_flags);
}

/* ---- the gather's second wire format on the host (k_gather.h): the layout arithmetic, and pack -> slots -> un-tile in plain loops over the functions the
 * kernels and comm_configure use.  No device needed. ---- */
static int gather_blocks(uint32_t width, uint32_t height, uint32_t world, std::vector<std::vector<uint32_t>> &orders, uint64_t *stride_out) {
    if (!width || !height || width > 65535u || height > 65535u || !world || world > 64u) { rpt_create_error() = "gather hooks: width / height must be in 1..65535, world in 1..64"; return RPT_EINVAL; }
    orders.assign(world, {});
    uint64_t stride = 0;
    for (uint32_t r = 0; r < world; ++r) {
        rpt_build_pixel_order(width, height, r, world, orders[r]);
        stride = std::max<uint64_t>(stride, orders[r].size());
    }
    *stride_out = stride;
    return RPT_OK;
}

int rpt_debug_gather_layout(uint32_t width, uint32_t height, uint32_t world, uint32_t with_moments, uint64_t *stride_pixels_out, uint64_t *slot_floats_out,
                            uint64_t *block_pixels_out, uint64_t *message_floats_out) {
    std::vector<std::vector<uint32_t>> orders;
    uint64_t stride = 0;
    RPT_TRY(gather_blocks(width, height, world, orders, &stride));
    const GatherLayout lay = gather_layout(stride, with_moments);
    if (stride_pixels_out) *stride_pixels_out = lay.stride;
    if (slot_floats_out) *slot_floats_out = lay.slot * 4u;
    for (uint32_t r = 0; r < world; ++r) {
        if (block_pixels_out) block_pixels_out[r] = orders[r].size();
        if (message_floats_out) message_floats_out[r] = gather_message(lay, orders[r].size(), with_moments) * 4u;
    }
    return RPT_OK;
}

int rpt_debug_gather_host(uint32_t width, uint32_t height, uint32_t world, const float *accum_blocks, const float *moments_blocks, const uint32_t *trailers,
                          float *slots_io, float *image_out, float *moments_out, rpt_gathered_info *info_out) {
    if (!accum_blocks || !moments_blocks || !trailers) { rpt_create_error() = "rpt_debug_gather_host: null blocks or trailers"; return RPT_EINVAL; }
    std::vector<std::vector<uint32_t>> orders;
    uint64_t stride = 0;
    RPT_TRY(gather_blocks(width, height, world, orders, &stride));
    const GatherLayout lay = gather_layout(stride, 1u);
    std::vector<float> own;
    if (!slots_io) { own.assign((size_t)world * lay.slot * 4u, 0.0f); slots_io = own.data(); }      /* (zeroed when they are sized) */
    /* k_gather_pack, rank by rank: the two records of every owned pixel and the trailer; the padding behind a block is not touched */
    size_t first = 0;
    for (uint32_t r = 0; r < world; ++r) {
        float *slot = slots_io + (size_t)r * lay.slot * 4u;
        const size_t n = orders[r].size();
        memcpy(slot, accum_blocks + first * 4u, n * 4u * sizeof(float));
        memcpy(slot + lay.moments_at * 4u, moments_blocks + first * 4u, n * 4u * sizeof(float));
        memcpy(slot + lay.trailer_at * 4u, trailers + (size_t)r * 4u, 4u * sizeof(uint32_t));
        first += n;
    }
    /* k_gather_untile2: the map is the orders padded to the stride */
    rpt_gathered_info g = gather_info_begin();
    for (uint32_t r = 0; r < world; ++r) {
        const float *slot = slots_io + (size_t)r * lay.slot * 4u;
        uint4 t;
        memcpy(&t, slot + lay.trailer_at * 4u, sizeof t);
        gather_fold(g, t);
        for (size_t i = 0; i < orders[r].size(); ++i) {
            const size_t at = rpt_pixel_index(orders[r][i], width) * 4u;
            if (image_out) memcpy(image_out + at, slot + i * 4u, 4u * sizeof(float));
            if (moments_out) memcpy(moments_out + at, slot + (lay.moments_at + i) * 4u, 4u * sizeof(float));
        }
    }
    gather_info_end(g);
    if (info_out) *info_out = g;
    return RPT_OK;
}

}  // extern "C"
