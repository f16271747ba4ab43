// upscale_kernel.hip -- G-buffer-guided upscaling of include/dsrt.h (UPSCALER): two kernels.
//
//   pack      one thread per LOW-resolution pixel: everything a tap reads packed into 16-byte records, as the denoiser's prepare kernel does, so that a tap is
//             one dwordx4 load to decide whether it counts and four more when it does:
//                 cr = {c.rgb, range}   vf = {v.rgb, flags (the byte, as a bit pattern)}   nn = {N, 0}   xx = {X, 0}   aa = {A, 0}
//             (v = 0 without a variance input, flags = 0 without the flags channel)
//   upscale   one lane per OUTPUT pixel, 16 x 16 pixels per workgroup: the pixel's own full-resolution guides, the 4 x 4 low-resolution taps gathered straight
//             through L1 / L2 (the s^2 output pixels over one low-resolution pixel share its sixteen taps, and a workgroup's footprint is (16/s + 3)^2 records
//             per array), both levels of the header in its order (qy outer, qx inner, one accumulator per sum: nothing is reassociated, a skipped tap is a
//             branch), then the tone map and 8-bit store (pixel_arith.h); templated over where powf comes from (DsrtRenderDesc.math_mode).
//
// With coverage (include/dsrt.h, COVERAGE-AWARE UPSCALER) both kernels have a second instantiation behind a symbol of its own, HAS_ALPHA = true of the same bodies;
// HAS_ALPHA = false is the kernel above, instruction for instruction.  pack then stores the low-resolution alpha in nn.w, and the gather divides every usable tap's
// colour by it (per tap, as the header writes it), weighs the tap by it, falls back over the usable taps alone before the tent over all of them, and multiplies by
// the output pixel's own alpha.
//
// Every index is bounded where it is formed: a tap is read only when 0 <= qx < w and 0 <= qy < h, an output pixel is processed only when X < W and Y < H.
// There is no reference counterpart: the reference upscales outside the renderer (src/main.cpp:194-215 shells out to a learned upscaler).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, no fast-math -- IEEE division and the absence of contraction are the contract.
#include <cfloat>

#include "../../include/dsrt.h"
#include "launchers.h"
#include "pixel_arith.h"

namespace dsrt {

// pack's body, over "has alpha": HAS_ALPHA = false is the plain upscaler's kernel, instruction for instruction.
template <bool HAS_ALPHA>
__device__ __forceinline__ void up_pack(const float* __restrict__ linear, const float* __restrict__ var, const float* __restrict__ normal, const float* __restrict__ position,
                                        const float* __restrict__ albedo, const float* __restrict__ range, const uint8_t* __restrict__ flags, const float* __restrict__ alpha,
                                        size_t n_pixels, float4* __restrict__ cr, float4* __restrict__ vf, float4* __restrict__ nn, float4* __restrict__ xx,
                                        float4* __restrict__ aa) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const float f = __uint_as_float(flags ? (uint32_t)flags[i] : 0u);
    float al = 0.0f;
    if constexpr (HAS_ALPHA) al = alpha[i];
    cr[i] = make_float4(linear[i * 3 + 0], linear[i * 3 + 1], linear[i * 3 + 2], range[i]);
    vf[i] = var ? make_float4(var[i * 3 + 0], var[i * 3 + 1], var[i * 3 + 2], f) : make_float4(0.0f, 0.0f, 0.0f, f);
    nn[i] = make_float4(normal[i * 3 + 0], normal[i * 3 + 1], normal[i * 3 + 2], al);
    xx[i] = make_float4(position[i * 3 + 0], position[i * 3 + 1], position[i * 3 + 2], 0.0f);
    aa[i] = make_float4(albedo[i * 3 + 0], albedo[i * 3 + 1], albedo[i * 3 + 2], 0.0f);
}

__global__ __launch_bounds__(256) void dsrt_upscale_pack_kernel(const float* __restrict__ linear, const float* __restrict__ var, const float* __restrict__ normal,
                                                                const float* __restrict__ position, const float* __restrict__ albedo, const float* __restrict__ range,
                                                                const uint8_t* __restrict__ flags, size_t n_pixels, float4* __restrict__ cr, float4* __restrict__ vf,
                                                                float4* __restrict__ nn, float4* __restrict__ xx, float4* __restrict__ aa) {
    up_pack<false>(linear, var, normal, position, albedo, range, flags, nullptr, n_pixels, cr, vf, nn, xx, aa);
}

__global__ __launch_bounds__(256) void dsrt_upscale_pack_coverage_kernel(const float* __restrict__ linear, const float* __restrict__ var, const float* __restrict__ normal,
                                                                         const float* __restrict__ position, const float* __restrict__ albedo,
                                                                         const float* __restrict__ range, const uint8_t* __restrict__ flags, const float* __restrict__ alpha,
                                                                         size_t n_pixels, float4* __restrict__ cr, float4* __restrict__ vf, float4* __restrict__ nn,
                                                                         float4* __restrict__ xx, float4* __restrict__ aa) {
    up_pack<true>(linear, var, normal, position, albedo, range, flags, alpha, n_pixels, cr, vf, nn, xx, aa);
}

// The gather: one output pixel per lane (upscale_pixel_body.h), without and with coverage.
template <bool DEVICE_LIBM>
__global__ __launch_bounds__(256) void dsrt_upscale_kernel(const UpscaleArgs a) {
    constexpr bool HAS_ALPHA = false;
    const float* const hi_alpha = nullptr;
    const float alpha_min = 0.0f;
    uint8_t* const out_level = nullptr;
#include "upscale_pixel_body.h"
}

template <bool DEVICE_LIBM>
__global__ __launch_bounds__(256) void dsrt_upscale_coverage_kernel(const UpscaleCoverageArgs ca) {
    constexpr bool HAS_ALPHA = true;
    const UpscaleArgs& a = ca.up;
    const float* __restrict__ const hi_alpha = ca.hi_alpha;
    const float alpha_min = ca.alpha_min;
    uint8_t* __restrict__ const out_level = ca.out_level;
#include "upscale_pixel_body.h"
}

hipError_t launch_upscale_pack(const float* linear, const float* var, const float* normal, const float* position, const float* albedo, const float* range,
                               const uint8_t* flags, size_t n_pixels, const UpscaleRecords& r, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_upscale_pack_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, linear, var, normal, position, albedo, range, flags,
                       n_pixels, r.cr, r.vf, r.nn, r.xx, r.aa);
    return hipGetLastError();
}

hipError_t launch_upscale_pack_coverage(const float* linear, const float* var, const float* normal, const float* position, const float* albedo, const float* range,
                                        const uint8_t* flags, const float* alpha, size_t n_pixels, const UpscaleRecords& r, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_upscale_pack_coverage_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, linear, var, normal, position, albedo, range,
                       flags, alpha, n_pixels, r.cr, r.vf, r.nn, r.xx, r.aa);
    return hipGetLastError();
}

hipError_t launch_upscale(const UpscaleArgs& a, bool device_libm, hipStream_t stream) {
    const dim3 grid((unsigned)((a.W + 15) / 16), (unsigned)((a.H + 15) / 16));
    if (device_libm) hipLaunchKernelGGL(dsrt_upscale_kernel<true>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(dsrt_upscale_kernel<false>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_upscale_coverage(const UpscaleCoverageArgs& a, bool device_libm, hipStream_t stream) {
    const dim3 grid((unsigned)((a.up.W + 15) / 16), (unsigned)((a.up.H + 15) / 16));
    if (device_libm) hipLaunchKernelGGL(dsrt_upscale_coverage_kernel<true>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(dsrt_upscale_coverage_kernel<false>, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dsrt
