/*
 * k_image_order.h — out of the tile-major pixel order into a row-major W x H image.  A context keeps its per-pixel data (accumulator, rng, moments) in the
 * order of its rank's pixel_xy (k_common.h rpt_pixel_index); whatever hands an image to the caller scatters with the ONE kernel below, which owns the
 * range check, the map load, the padding skip and the index and leaves what is stored to an operation.  rpt_read_out is the read-out built on it
 * (rpt_read_rng, rpt_resolve, rpt_read_moments, rpt_read_noise); the accumulator read-back and the gather (rpt_comm.hip) keep their persistent buffers
 * and streams and share the kernel.  Each translation unit that includes the header instantiates the kernels it launches.
 */
#ifndef RPT_K_IMAGE_ORDER_H
#define RPT_K_IMAGE_ORDER_H

#include <type_traits>

#include "rpt_ctx.h"
#include "k_moments.h"
#include "k_tonemap.h"

/* element i of the operation's source belongs to pixel map[i] = x | y << 16 (0xffffffff: padding between the blocks of a gather, nobody's): op(i, its row-major index) */
template <typename Op>
static __global__ __launch_bounds__(RPT_BLOCK) void k_scatter_pixels(const uint32_t *map, uint32_t n, uint32_t width, Op op) {
    const uint32_t i = blockIdx.x * RPT_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t pxy = map[i];
    if (pxy == 0xffffffffu) return;
    op(i, rpt_pixel_index(pxy, width));
}

/* The operations: `image` is the destination, per_pixel its elements per pixel (what rpt_read_out sizes it by). */
/* a copy: float4 (accumulator blocks, moments records) and uint2 (rng states) */
template <typename T> struct PixelCopy {
    static constexpr size_t per_pixel = 1;
    const T *src;
    T *image;
    __device__ void operator()(uint32_t i, size_t at) const { image[at] = src[i]; }
};
/* noise_rel of a moments record (k_moments.h) */
struct PixelNoise {
    static constexpr size_t per_pixel = 1;
    const float4 *moments;
    float *image;
    __device__ void operator()(uint32_t i, size_t at) const { image[at] = noise_rel(moments[i]); }
};
/* The post-accumulation step: mean = sum / sample_count (src/trace.rs:199-204) followed by one of the display tonemappers of
 * src/resources/render.wgsl:36-117 (operator selection :131-153; the curves: k_tonemap.h, shared with the denoiser and its host build), as RGB. */
struct PixelResolve {
    static constexpr size_t per_pixel = 3;
    const float4 *accum;
    float sample_count;
    uint32_t op;
    float *image;
    __device__ void operator()(uint32_t i, size_t at) const {
        const float4 a = accum[i];
        const F3 mean = f3(a.x / sample_count, a.y / sample_count, a.z / sample_count);
        const F3 c = tonemap(op, mean);
        float *rgb = image + 3u * at;
        rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
    }
};

/* One read-out: a temporary row-major image of W x H x Op::per_pixel elements, zeroed (other ranks' pixels stay 0), filled by `op` from the rank's
 * n_pixels (op.image is set here), copied to `out`.  Everything is enqueued on the context's stream behind what is there already and completed by
 * rpt_wait — so EVERY read-out, rpt_resolve and rpt_read_rng included, also verifies that an asynchronous batch drained, and reports one that did not. */
template <typename Op>
int rpt_read_out(rpt_ctx *c, Op op, void *out) {
    using T = std::remove_pointer_t<decltype(op.image)>;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->cfg.c.width * c->cfg.c.height * Op::per_pixel;
    DevBuf<T> image;
    HIP_TRY(c, image.alloc(n));
    HIP_TRY(c, hipMemsetAsync(image.p, 0, n * sizeof(T), c->stream));
    op.image = image.p;
    if (c->n_pixels) k_scatter_pixels<<<rpt_blocks(c->n_pixels), RPT_BLOCK, 0, c->stream>>>(c->pixel_xy.p, c->n_pixels, c->cfg.c.width, op);
    HIP_TRY(c, hipGetLastError());
    RPT_TRY(rpt_wait(c));
    HIP_TRY(c, hipMemcpy(out, image.p, n * sizeof(T), hipMemcpyDeviceToHost));
    return RPT_OK;
}

#endif /* RPT_K_IMAGE_ORDER_H */
