// pixel_arith.h -- the arithmetic between a pixel's integer sums and its bytes, which include/dsrt.h pins bit for bit, stated once for every kernel that resolves,
// filters or stores a pixel.  Each function names the line of the header it implements.  The double operations are correctly rounded + - * / and conversions only
// (-ffp-contract=off, no sqrt), so that a CPU reproduces every bit.
#pragma once

#include "device_math.h"

namespace dsrt {

constexpr double kSumUnit = 1.0 / 1048576.0;             // dsrt.h:318  a pixel's samples are summed as integers in units of 2^-20

// dsrt.h:330  (float)((double)sum * (1.0 / 2^20 / n)), computed in double and converted to float once
__device__ __forceinline__ float sum_mean(unsigned long long sum, double n) {
    const double unit = kSumUnit / n;
    return (float)((double)sum * unit);
}

// dsrt.h:345  s = (double)S * 2^-20;  s2 = (double)S2 * 2^-20;  v = (s2 - s * s / n) / (n - 1);  v = v > 0 ? v : 0.  The caller divides by n (the variance of the
// mean); `s` goes back too: the convergence test (dsrt.h:657) takes m = s / n from the same s.  n >= 2 is the caller's to ensure.
__device__ __forceinline__ double sum_variance(unsigned long long sum, unsigned long long sum_sq, double n, double& s) {
    s = (double)sum * kSumUnit;
    const double s2 = (double)sum_sq * kSumUnit;
    const double v = (s2 - s * s / n) / (n - 1.0);
    return v > 0.0 ? v : 0.0;
}

// dsrt.h:331  clamp to [0,10], pow(1/gamma), clamp to [0,1] (the reference's :1003-1030).  DEVICE_LIBM: the device math library's powf (math_mode 1), otherwise
// include/dsrt_detmath.h's.  Two spellings of the same operations per channel, because the compiler schedules them differently and the kernels are held to their
// instructions (tools/device_code_diff.py): one channel through every step (the reconstruction filters' output kernels), and all three channels through each
// step in turn (the render kernels and the resolve).
template <bool DEVICE_LIBM>
__device__ __forceinline__ float tone_map(float c, float inv_gamma) {
    c = fminf(fmaxf(c, 0.0f), 10.0f);
    c = DEVICE_LIBM ? ::powf(c, inv_gamma) : dsrt_powf(c, inv_gamma);
    return fminf(1.0f, fmaxf(0.0f, c));
}
template <bool DEVICE_LIBM>
__device__ __forceinline__ F3 tone_map(F3 col, float inv_gamma) {
    col = mk(fmaxf(col.x, 0.0f), fmaxf(col.y, 0.0f), fmaxf(col.z, 0.0f));
    col = mk(fminf(col.x, 10.0f), fminf(col.y, 10.0f), fminf(col.z, 10.0f));
    if constexpr (DEVICE_LIBM) col = mk(::powf(col.x, inv_gamma), ::powf(col.y, inv_gamma), ::powf(col.z, inv_gamma));
    else col = mk(dsrt_powf(col.x, inv_gamma), dsrt_powf(col.y, inv_gamma), dsrt_powf(col.z, inv_gamma));
    return clamp01(col);
}

// dsrt.h:331  the 8-bit store, (unsigned char)(255.99 * c), three bytes from out[o].  `out` is a reference so that a pointer the caller keeps in memory (the render
// kernels' argument segment) is read where each byte is stored, after its product, as the plain statement reads it: the render kernels' instruction order depends
// on it.  __restrict lets it bind to the tail kernels' restrict-qualified parameters as well.
__device__ __forceinline__ void store_rgb8(uint8_t* const __restrict& out, size_t o, F3 col) {
    out[o + 0] = (unsigned char)(255.99f * col.x);
    out[o + 1] = (unsigned char)(255.99f * col.y);
    out[o + 2] = (unsigned char)(255.99f * col.z);
}

// dsrt.h:702  L(x) = (0.2126f*x.r + 0.7152f*x.g) + 0.0722f*x.b        dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z
__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }

}  // namespace dsrt
