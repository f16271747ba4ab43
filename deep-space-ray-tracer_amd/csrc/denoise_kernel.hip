// denoise_kernel.hip -- the variance-guided a-trous filter of include/dsrt.h (DENOISER): three kernels, one thread per pixel each.
//
//   prepare   mean and variance of the mean from the integer sums (pixel_arith.h: the resolve's own functions), and everything a tap
//             reads packed into 16-byte records, so that a tap is five dwordx4 loads:
//                 cl = {c.rgb, L(c)}   vl = {v.rgb, L(v)}   nr = {N, range}   xf = {X, F ? 1 : 0}   al = {A, 0}
//             L(c) and L(v) are cached beside the values they are the luminance of: computed once, by the operations the header writes, wherever c and v are written.
//   a-trous   one launch per iteration, cl / vl ping-ponging; 16 x 16 pixels per workgroup.  The sums run in the header's order (dy outer, dx inner, one
//             accumulator each): nothing is reassociated, a skipped tap is a branch.
//   output    d_linear, d_var and the tone map + 8-bit store (pixel_arith.h) of the filtered mean; templated over where powf comes from (DsrtRenderDesc.math_mode).
// prepare and output are bodies templated over "has alpha" (include/dsrt.h, COVERAGE DEMODULATION: dsrt_denoise_accumulated_coverage) behind two kernels each:
// the plain denoiser's, unchanged instruction for instruction, and the _coverage ones, which divide the filterable pixels' c and v by alpha and alpha^2 at the
// start and multiply them back at the end.
//
// There is no reference counterpart: the reference reconstructs its 250-spp frames outside the renderer (scripts/upsample.py).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, no fast-math -- IEEE division and square root and the absence of contraction are the contract.
#include <cfloat>

#include "launchers.h"
#include "pixel_arith.h"

namespace dsrt {

// prepare's body, over "has alpha" (include/dsrt.h, COVERAGE DEMODULATION): HAS_ALPHA = false is the plain denoiser's kernel, instruction for instruction.
template <bool HAS_ALPHA>
__device__ __forceinline__ void denoise_prepare(const unsigned long long* __restrict__ sums, const unsigned long long* __restrict__ sums_sq, int samples_done,
                                                const uint32_t* __restrict__ counts, const float* __restrict__ normal, const float* __restrict__ position,
                                                const float* __restrict__ albedo, const float* __restrict__ range, const float* __restrict__ alpha, float alpha_min,
                                                size_t n_pixels, float4* __restrict__ cl, float4* __restrict__ vl, float4* __restrict__ nr, float4* __restrict__ xf,
                                                float4* __restrict__ al) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    const uint32_t cnt = counts ? counts[i] : (uint32_t)samples_done;
    float c[3] = {0.0f, 0.0f, 0.0f}, v[3] = {0.0f, 0.0f, 0.0f};
    if (cnt) {
        for (int ch = 0; ch < 3; ++ch) c[ch] = sum_mean(sums[i * 3 + ch], (double)cnt);
    }
    if (cnt >= 2u) {
        const double n = (double)cnt;
        for (int ch = 0; ch < 3; ++ch) {
            double s;
            v[ch] = (float)(sum_variance(sums[i * 3 + ch], sums_sq[i * 3 + ch], n, s) / n);
        }
    }
    const float r = range[i];
    bool filterable = r <= FLT_MAX && cnt >= 2u;                       // false for a NaN range
    if constexpr (HAS_ALPHA) {
        const float a = alpha[i];
        filterable = filterable && a >= alpha_min;                     // false for a NaN alpha
        if (filterable) {
            const float aa = a * a;
            for (int ch = 0; ch < 3; ++ch) { c[ch] = c[ch] / a; v[ch] = v[ch] / aa; }
        }
    }
    cl[i] = make_float4(c[0], c[1], c[2], lum(c[0], c[1], c[2]));
    vl[i] = make_float4(v[0], v[1], v[2], lum(v[0], v[1], v[2]));
    nr[i] = make_float4(normal[i * 3 + 0], normal[i * 3 + 1], normal[i * 3 + 2], r);
    xf[i] = make_float4(position[i * 3 + 0], position[i * 3 + 1], position[i * 3 + 2], filterable ? 1.0f : 0.0f);
    al[i] = make_float4(albedo[i * 3 + 0], albedo[i * 3 + 1], albedo[i * 3 + 2], 0.0f);
}

__global__ __launch_bounds__(256) void dsrt_denoise_prepare_kernel(const unsigned long long* __restrict__ sums, const unsigned long long* __restrict__ sums_sq, int samples_done,
                                                                   const uint32_t* __restrict__ counts, const float* __restrict__ normal, const float* __restrict__ position,
                                                                   const float* __restrict__ albedo, const float* __restrict__ range, size_t n_pixels,
                                                                   float4* __restrict__ cl, float4* __restrict__ vl, float4* __restrict__ nr, float4* __restrict__ xf,
                                                                   float4* __restrict__ al) {
    denoise_prepare<false>(sums, sums_sq, samples_done, counts, normal, position, albedo, range, nullptr, 0.0f, n_pixels, cl, vl, nr, xf, al);
}

__global__ __launch_bounds__(256) void dsrt_denoise_prepare_coverage_kernel(const unsigned long long* __restrict__ sums, const unsigned long long* __restrict__ sums_sq,
                                                                            int samples_done, const uint32_t* __restrict__ counts, const float* __restrict__ normal,
                                                                            const float* __restrict__ position, const float* __restrict__ albedo,
                                                                            const float* __restrict__ range, const float* __restrict__ alpha, float alpha_min, size_t n_pixels,
                                                                            float4* __restrict__ cl, float4* __restrict__ vl, float4* __restrict__ nr, float4* __restrict__ xf,
                                                                            float4* __restrict__ al) {
    denoise_prepare<true>(sums, sums_sq, samples_done, counts, normal, position, albedo, range, alpha, alpha_min, n_pixels, cl, vl, nr, xf, al);
}

__global__ __launch_bounds__(256) void dsrt_denoise_atrous_kernel(const float4* __restrict__ cl_in, const float4* __restrict__ vl_in, const float4* __restrict__ nr,
                                                                  const float4* __restrict__ xf, const float4* __restrict__ al, float4* __restrict__ cl_out,
                                                                  float4* __restrict__ vl_out, int W, int H, int step, int normal_power_log2, float sigma_l, float sigma_z,
                                                                  float sigma_a) {
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const float4 cp = cl_in[p], vp = vl_in[p], xp = xf[p];
    if (xp.w == 0.0f) { cl_out[p] = cp; vl_out[p] = vp; return; }        // not filterable: copied through, bit for bit

    constexpr float k3[3] = {0.25f, 0.5f, 0.25f};
    constexpr float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float g = 0.0f;
    for (int ey = -1; ey <= 1; ++ey) {
        const int qy = min(max(y + ey, 0), H - 1);
#pragma unroll
        for (int ex = -1; ex <= 1; ++ex) {
            const int qx = min(max(x + ex, 0), W - 1);
            g += (k3[ex + 1] * k3[ey + 1]) * vl_in[(size_t)qy * (size_t)W + (size_t)qx].w;
        }
    }
    const float4 np = nr[p], ap = al[p];
    const float den_l = sigma_l * sqrtf(g) + 0x1p-20f;
    const float den_z = sigma_z * np.w;
    const float sa2 = sigma_a * sigma_a;
    const float lp = cp.w;

    float sw = 0.0f, sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f, sv0 = 0.0f, sv1 = 0.0f, sv2 = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + step * dy;
        if (qy < 0 || qy >= H) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + step * dx;
            if (qx < 0 || qx >= W) continue;
            const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
            const float4 xq = xf[q];
            if (xq.w == 0.0f) continue;
            const float4 nq = nr[q], cq = cl_in[q], vq = vl_in[q], aq = al[q];
            float wn = fmaxf(dot3(np.x, np.y, np.z, nq.x, nq.y, nq.z), 0.0f);
            for (int k = 0; k < normal_power_log2; ++k) wn = wn * wn;
            const float ez = fabsf(dot3(np.x, np.y, np.z, xq.x - xp.x, xq.y - xp.y, xq.z - xp.z)) / den_z;
            const float el = fabsf(cq.w - lp) / den_l;
            const float dax = aq.x - ap.x, day = aq.y - ap.y, daz = aq.z - ap.z;
            const float ea2 = dot3(dax, day, daz, dax, day, daz) / sa2;
            const float w = ((h[dx + 2] * h[dy + 2]) * wn) / (((1.0f + ez * ez) * (1.0f + el * el)) * (1.0f + ea2));
            const float w2 = w * w;
            sw += w;
            sc0 += w * cq.x; sc1 += w * cq.y; sc2 += w * cq.z;
            sv0 += w2 * vq.x; sv1 += w2 * vq.y; sv2 += w2 * vq.z;
        }
    }
    if (sw > 0.0f) {
        const float sw2 = sw * sw;
        const float c0 = sc0 / sw, c1 = sc1 / sw, c2 = sc2 / sw, v0 = sv0 / sw2, v1 = sv1 / sw2, v2 = sv2 / sw2;
        cl_out[p] = make_float4(c0, c1, c2, lum(c0, c1, c2));
        vl_out[p] = make_float4(v0, v1, v2, lum(v0, v1, v2));
    } else {
        cl_out[p] = cp;
        vl_out[p] = vp;
    }
}

// output's body, over "has alpha": the filterable pixels' c and v multiplied back by a and a*a (xf.w is prepare's F_p, alpha_min included) before anything is written.
template <bool DEVICE_LIBM, bool HAS_ALPHA>
__device__ __forceinline__ void denoise_output(const float4* __restrict__ cl, const float4* __restrict__ vl, const float4* __restrict__ xf, const float* __restrict__ alpha,
                                               size_t n_pixels, float inv_gamma, uint8_t* __restrict__ out_rgb8, float* __restrict__ out_f32, float* __restrict__ out_linear,
                                               float* __restrict__ out_var) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    float4 c = cl[i];
    float a = 1.0f;
    bool scaled = false;
    if constexpr (HAS_ALPHA) {
        scaled = xf[i].w != 0.0f;
        if (scaled) { a = alpha[i]; c.x = c.x * a; c.y = c.y * a; c.z = c.z * a; }
    }
    if (out_linear) { out_linear[i * 3 + 0] = c.x; out_linear[i * 3 + 1] = c.y; out_linear[i * 3 + 2] = c.z; }
    if (out_var) {
        float4 v = vl[i];
        if constexpr (HAS_ALPHA) { if (scaled) { const float aa = a * a; v.x = v.x * aa; v.y = v.y * aa; v.z = v.z * aa; } }
        out_var[i * 3 + 0] = v.x; out_var[i * 3 + 1] = v.y; out_var[i * 3 + 2] = v.z;
    }
    if (!out_rgb8 && !out_f32) return;
    const F3 col = mk(tone_map<DEVICE_LIBM>(c.x, inv_gamma), tone_map<DEVICE_LIBM>(c.y, inv_gamma), tone_map<DEVICE_LIBM>(c.z, inv_gamma));
    if (out_rgb8) store_rgb8(out_rgb8, i * 3, col);
    if (out_f32) { out_f32[i * 3 + 0] = col.x; out_f32[i * 3 + 1] = col.y; out_f32[i * 3 + 2] = col.z; }
}

template <bool DEVICE_LIBM>
__global__ __launch_bounds__(256) void dsrt_denoise_output_kernel(const float4* __restrict__ cl, const float4* __restrict__ vl, size_t n_pixels, float inv_gamma,
                                                                  uint8_t* __restrict__ out_rgb8, float* __restrict__ out_f32, float* __restrict__ out_linear,
                                                                  float* __restrict__ out_var) {
    denoise_output<DEVICE_LIBM, false>(cl, vl, nullptr, nullptr, n_pixels, inv_gamma, out_rgb8, out_f32, out_linear, out_var);
}

template <bool DEVICE_LIBM>
__global__ __launch_bounds__(256) void dsrt_denoise_output_coverage_kernel(const float4* __restrict__ cl, const float4* __restrict__ vl, const float4* __restrict__ xf,
                                                                           const float* __restrict__ alpha, size_t n_pixels, float inv_gamma, uint8_t* __restrict__ out_rgb8,
                                                                           float* __restrict__ out_f32, float* __restrict__ out_linear, float* __restrict__ out_var) {
    denoise_output<DEVICE_LIBM, true>(cl, vl, xf, alpha, n_pixels, inv_gamma, out_rgb8, out_f32, out_linear, out_var);
}

hipError_t launch_denoise_prepare(const unsigned long long* sums, const unsigned long long* sums_sq, int samples_done, const uint32_t* counts, const float* normal,
                                  const float* position, const float* albedo, const float* range, size_t n_pixels, const DenoiseBuffers& b, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_denoise_prepare_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, sums, sums_sq, samples_done, counts, normal, position,
                       albedo, range, n_pixels, b.cl[0], b.vl[0], b.nr, b.xf, b.al);
    return hipGetLastError();
}

hipError_t launch_denoise_prepare_coverage(const unsigned long long* sums, const unsigned long long* sums_sq, int samples_done, const uint32_t* counts, const float* normal,
                                           const float* position, const float* albedo, const float* range, const float* alpha, float alpha_min, size_t n_pixels,
                                           const DenoiseBuffers& b, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_denoise_prepare_coverage_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, sums, sums_sq, samples_done, counts, normal,
                       position, albedo, range, alpha, alpha_min, n_pixels, b.cl[0], b.vl[0], b.nr, b.xf, b.al);
    return hipGetLastError();
}

hipError_t launch_denoise_atrous(const DenoiseBuffers& b, int src, int W, int H, int step, int normal_power_log2, float sigma_l, float sigma_z, float sigma_a,
                                 hipStream_t stream) {
    const dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 15) / 16));
    hipLaunchKernelGGL(dsrt_denoise_atrous_kernel, grid, dim3(256), 0, stream, b.cl[src], b.vl[src], b.nr, b.xf, b.al, b.cl[src ^ 1], b.vl[src ^ 1], W, H, step,
                       normal_power_log2, sigma_l, sigma_z, sigma_a);
    return hipGetLastError();
}

hipError_t launch_denoise_output(const DenoiseBuffers& b, int src, size_t n_pixels, float inv_gamma, bool device_libm, uint8_t* out_rgb8, float* out_f32, float* out_linear,
                                 float* out_var, hipStream_t stream) {
    const dim3 grid((unsigned)((n_pixels + 255) / 256)), block(256);
    if (device_libm) hipLaunchKernelGGL(dsrt_denoise_output_kernel<true>, grid, block, 0, stream, b.cl[src], b.vl[src], n_pixels, inv_gamma, out_rgb8, out_f32, out_linear, out_var);
    else hipLaunchKernelGGL(dsrt_denoise_output_kernel<false>, grid, block, 0, stream, b.cl[src], b.vl[src], n_pixels, inv_gamma, out_rgb8, out_f32, out_linear, out_var);
    return hipGetLastError();
}

hipError_t launch_denoise_output_coverage(const DenoiseBuffers& b, int src, const float* alpha, size_t n_pixels, float inv_gamma, bool device_libm, uint8_t* out_rgb8,
                                          float* out_f32, float* out_linear, float* out_var, hipStream_t stream) {
    const dim3 grid((unsigned)((n_pixels + 255) / 256)), block(256);
    if (device_libm) hipLaunchKernelGGL(dsrt_denoise_output_coverage_kernel<true>, grid, block, 0, stream, b.cl[src], b.vl[src], b.xf, alpha, n_pixels, inv_gamma, out_rgb8, out_f32, out_linear, out_var);
    else hipLaunchKernelGGL(dsrt_denoise_output_coverage_kernel<false>, grid, block, 0, stream, b.cl[src], b.vl[src], b.xf, alpha, n_pixels, inv_gamma, out_rgb8, out_f32, out_linear, out_var);
    return hipGetLastError();
}

}  // namespace dsrt
