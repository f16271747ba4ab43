// upscale_kernel.hip -- G-buffer-guided upscaling of include/dsrt.h (UPSCALER): two kernels.
//
//   pack      one thread per LOW-resolution pixel: everything a tap reads packed into 16-byte records, as the denoiser's prepare kernel does, so that a tap is
//             one dwordx4 load to decide whether it counts and four more when it does:
//                 cr = {c.rgb, range}   vf = {v.rgb, flags (the byte, as a bit pattern)}   nn = {N, 0}   xx = {X, 0}   aa = {A, 0}
//             (v = 0 without a variance input, flags = 0 without the flags channel)
//   upscale   one lane per OUTPUT pixel, 16 x 16 pixels per workgroup: the pixel's own full-resolution guides, the 4 x 4 low-resolution taps gathered straight
//             through L1 / L2 (the s^2 output pixels over one low-resolution pixel share its sixteen taps, and a workgroup's footprint is (16/s + 3)^2 records
//             per array), both levels of the header in its order (qy outer, qx inner, one accumulator per sum: nothing is reassociated, a skipped tap is a
//             branch), then the resolve's tone map and 8-bit store; templated over where powf comes from (DsrtRenderDesc.math_mode).
//
// Every index is bounded where it is formed: a tap is read only when 0 <= qx < w and 0 <= qy < h, an output pixel is processed only when X < W and Y < H.
// There is no reference counterpart: the reference upscales outside the renderer (src/main.cpp:194-215 shells out to a learned upscaler).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, no fast-math -- IEEE division and the absence of contraction are the contract.
#include <cfloat>

#include "../../include/dsrt.h"
#include "../../include/dsrt_detmath.h"
#include "launchers.h"

namespace dsrt {

namespace {
__device__ __forceinline__ float up_dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

template <bool DEVICE_LIBM>
__device__ __forceinline__ float up_tone(float c, float inv_gamma) {    // the resolve's tone map (render_kernel.hip, dsrt_resolve_kernel), operation for operation
    c = fminf(fmaxf(c, 0.0f), 10.0f);
    c = DEVICE_LIBM ? ::powf(c, inv_gamma) : dsrt_powf(c, inv_gamma);
    return fminf(1.0f, fmaxf(0.0f, c));
}
}  // namespace

__global__ __launch_bounds__(256) void dsrt_upscale_pack_kernel(const float* __restrict__ linear, const float* __restrict__ var, const float* __restrict__ normal,
                                                                const float* __restrict__ position, const float* __restrict__ albedo, const float* __restrict__ range,
                                                                const uint8_t* __restrict__ flags, size_t n_pixels, float4* __restrict__ cr, float4* __restrict__ vf,
                                                                float4* __restrict__ nn, float4* __restrict__ xx, float4* __restrict__ aa) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const float f = __uint_as_float(flags ? (uint32_t)flags[i] : 0u);
    cr[i] = make_float4(linear[i * 3 + 0], linear[i * 3 + 1], linear[i * 3 + 2], range[i]);
    vf[i] = var ? make_float4(var[i * 3 + 0], var[i * 3 + 1], var[i * 3 + 2], f) : make_float4(0.0f, 0.0f, 0.0f, f);
    nn[i] = make_float4(normal[i * 3 + 0], normal[i * 3 + 1], normal[i * 3 + 2], 0.0f);
    xx[i] = make_float4(position[i * 3 + 0], position[i * 3 + 1], position[i * 3 + 2], 0.0f);
    aa[i] = make_float4(albedo[i * 3 + 0], albedo[i * 3 + 1], albedo[i * 3 + 2], 0.0f);
}

template <bool DEVICE_LIBM>
__global__ __launch_bounds__(256) void dsrt_upscale_kernel(const UpscaleArgs a) {
    const int X = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), Y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    const int W = a.W, H = a.H, w = a.w, h = a.h;
    if (X >= W || Y >= H) return;
    const size_t P = (size_t)Y * (size_t)W + (size_t)X;
    const float R = a.hi_range[P];

    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, v0 = 0.0f, v1 = 0.0f, v2 = 0.0f, support = 0.0f;
    if (R <= FLT_MAX) {                                                  // false for a miss (+inf) and for a NaN
        const float fx = (((float)X + 0.5f) / (float)(W - 1)) * (float)(w - 1) - 0.5f;
        const float fyk = (((float)(H - 1 - Y) + 0.5f) / (float)(H - 1)) * (float)(h - 1) - 0.5f;
        const float fy = (float)(h - 1) - fyk;
        const int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
        const float npx = a.hi_normal[P * 3 + 0], npy = a.hi_normal[P * 3 + 1], npz = a.hi_normal[P * 3 + 2];
        const float xpx = a.hi_position[P * 3 + 0], xpy = a.hi_position[P * 3 + 1], xpz = a.hi_position[P * 3 + 2];
        const float apx = a.hi_albedo[P * 3 + 0], apy = a.hi_albedo[P * 3 + 1], apz = a.hi_albedo[P * 3 + 2];
        const bool sun = a.use_sun && a.hi_flags && a.lo_has_flags;
        const uint32_t fp = sun ? (uint32_t)a.hi_flags[P] : 0u;
        const float den_z = a.sigma_z * R;
        const float sa2 = a.sigma_a * a.sigma_a;

        float sw = 0.0f, sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f, sv0 = 0.0f, sv1 = 0.0f, sv2 = 0.0f;
        for (int qy = y0 - 1; qy <= y0 + 2; ++qy) {                      // level 1: the guided taps
            if (qy < 0 || qy >= h) continue;
            const float by = fmaxf(1.0f - 0.5f * fabsf((float)qy - fy), 0.0f);
#pragma unroll
            for (int dx = -1; dx <= 2; ++dx) {
                const int qx = x0 + dx;
                if (qx < 0 || qx >= w) continue;
                const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
                const float4 cq = a.cr[q];
                if (!(cq.w <= FLT_MAX)) continue;
                const float4 vq = a.vf[q];
                if (sun && ((__float_as_uint(vq.w) ^ fp) & (uint32_t)DSRT_GB_SUN_VISIBLE) != 0u) continue;
                const float4 nq = a.nn[q], xq = a.xx[q], aq = a.aa[q];
                const float bx = fmaxf(1.0f - 0.5f * fabsf((float)qx - fx), 0.0f);
                const float b = bx * by;
                float wn = fmaxf(up_dot3(npx, npy, npz, nq.x, nq.y, nq.z), 0.0f);
                for (int k = 0; k < a.normal_power_log2; ++k) wn = wn * wn;
                const float ez = fabsf(up_dot3(npx, npy, npz, xq.x - xpx, xq.y - xpy, xq.z - xpz)) / den_z;
                const float dax = aq.x - apx, day = aq.y - apy, daz = aq.z - apz;
                const float ea2 = up_dot3(dax, day, daz, dax, day, daz) / sa2;
                const float wt = (b * wn) / ((1.0f + ez * ez) * (1.0f + ea2));
                const float wt2 = wt * wt;
                sw += wt;
                sc0 += wt * cq.x; sc1 += wt * cq.y; sc2 += wt * cq.z;
                sv0 += wt2 * vq.x; sv1 += wt2 * vq.y; sv2 += wt2 * vq.z;
            }
        }
        support = sw;
        if (!(sw > 0.0f)) {                                              // level 2: every tap inside the image, the tent alone
            sw = 0.0f; sc0 = 0.0f; sc1 = 0.0f; sc2 = 0.0f; sv0 = 0.0f; sv1 = 0.0f; sv2 = 0.0f;
            support = 0.0f;
            for (int qy = y0 - 1; qy <= y0 + 2; ++qy) {
                if (qy < 0 || qy >= h) continue;
                const float by = fmaxf(1.0f - 0.5f * fabsf((float)qy - fy), 0.0f);
#pragma unroll
                for (int dx = -1; dx <= 2; ++dx) {
                    const int qx = x0 + dx;
                    if (qx < 0 || qx >= w) continue;
                    const size_t q = (size_t)qy * (size_t)w + (size_t)qx;
                    const float4 cq = a.cr[q], vq = a.vf[q];
                    const float bx = fmaxf(1.0f - 0.5f * fabsf((float)qx - fx), 0.0f);
                    const float wt = bx * by;
                    const float wt2 = wt * wt;
                    sw += wt;
                    sc0 += wt * cq.x; sc1 += wt * cq.y; sc2 += wt * cq.z;
                    sv0 += wt2 * vq.x; sv1 += wt2 * vq.y; sv2 += wt2 * vq.z;
                }
            }
        }
        const float sw2 = sw * sw;
        c0 = sc0 / sw; c1 = sc1 / sw; c2 = sc2 / sw;
        v0 = sv0 / sw2; v1 = sv1 / sw2; v2 = sv2 / sw2;
    }

    if (a.out_linear) { a.out_linear[P * 3 + 0] = c0; a.out_linear[P * 3 + 1] = c1; a.out_linear[P * 3 + 2] = c2; }
    if (a.out_var) { a.out_var[P * 3 + 0] = v0; a.out_var[P * 3 + 1] = v1; a.out_var[P * 3 + 2] = v2; }
    if (a.out_support) a.out_support[P] = support;
    if (!a.out_rgb8 && !a.out_f32) return;
    const float r = up_tone<DEVICE_LIBM>(c0, a.inv_gamma), g = up_tone<DEVICE_LIBM>(c1, a.inv_gamma), b = up_tone<DEVICE_LIBM>(c2, a.inv_gamma);
    if (a.out_rgb8) {
        a.out_rgb8[P * 3 + 0] = (unsigned char)(255.99f * r);
        a.out_rgb8[P * 3 + 1] = (unsigned char)(255.99f * g);
        a.out_rgb8[P * 3 + 2] = (unsigned char)(255.99f * b);
    }
    if (a.out_f32) { a.out_f32[P * 3 + 0] = r; a.out_f32[P * 3 + 1] = g; a.out_f32[P * 3 + 2] = b; }
}

hipError_t launch_upscale_pack(const float* linear, const float* var, const float* normal, const float* position, const float* albedo, const float* range,
                               const uint8_t* flags, size_t n_pixels, const UpscaleRecords& r, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_upscale_pack_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, linear, var, normal, position, albedo, range, flags,
                       n_pixels, r.cr, r.vf, r.nn, r.xx, r.aa);
    return hipGetLastError();
}

hipError_t launch_upscale(const UpscaleArgs& a, bool device_libm, hipStream_t stream) {
    const dim3 grid((unsigned)((a.W + 15) / 16), (unsigned)((a.H + 15) / 16));
    if (device_libm) hipLaunchKernelGGL(dsrt_upscale_kernel<true>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(dsrt_upscale_kernel<false>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dsrt
