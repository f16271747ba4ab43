// lens_math.h -- the arithmetic of include/dsrt.h's LENS MODEL, once: the forward model `distort`, the fixed-count inverse, the certificate, the source position and
// its window, the filters' weights and the vignetting gain.  Compiled by the kernel (csrc/lens_kernel.hip) and by the host (host/lens_host.cpp:
// dsrt_lens_distort_points), so that the label helper and the warp cannot drift apart; tests/_lens_model.py restates it in numpy and holds both to it bit for bit.
// Every operation is one correctly rounded IEEE fp32 operation in the order and parenthesisation written here: both builds use -ffp-contract=off and no fast-math,
// and `/` is the IEEE division on both sides.  Nothing here touches memory.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define DSRT_LENS_FN __host__ __device__ __forceinline__
#else
#define DSRT_LENS_FN inline
#endif

namespace dsrt {

constexpr int kLensIterations = 12;                 // the inverse's fixed-point steps: exactly this many, no early exit
constexpr float kLensCertificate = 0x1p-6f;         // the certificate's bound, in output pixels

struct LensCoeffs { float k1, k2, k3, p1, p2; };

// rad, dx, dy of the forward model at (xu, yu) -- step 2 of the header; distort() and the inverse both use exactly these.
DSRT_LENS_FN void lens_terms(const LensCoeffs& c, float xu, float yu, float& rad, float& dx, float& dy) {
    const float xx = xu * xu, yy = yu * yu, xy = xu * yu;
    const float r2 = xx + yy;
    rad = 1.0f + r2 * (c.k1 + r2 * (c.k2 + r2 * c.k3));
    dx = (2.0f * c.p1) * xy + c.p2 * (r2 + 2.0f * xx);
    dy = c.p1 * (r2 + 2.0f * yy) + (2.0f * c.p2) * xy;
}

DSRT_LENS_FN void lens_distort(const LensCoeffs& c, float xu, float yu, float& xr, float& yr) {
    float rad, dx, dy;
    lens_terms(c, xu, yu, rad, dx, dy);
    xr = xu * rad + dx;
    yr = yu * rad + dy;
}

// Step 3: kLensIterations steps of xu = (xd - dx(xu, yu)) / rad(xu, yu), both coordinates from the previous step's pair.
DSRT_LENS_FN void lens_undistort(const LensCoeffs& c, float xd, float yd, float& xu, float& yu) {
    xu = xd; yu = yd;
    for (int i = 0; i < kLensIterations; ++i) {
        float rad, dx, dy;
        lens_terms(c, xu, yu, rad, dx, dy);
        xu = (xd - dx) / rad;
        yu = (yd - dy) / rad;
    }
}

// Step 4: does the forward model bring (xu, yu) back to (xd, yd) within kLensCertificate output pixels?  A NaN fails.
DSRT_LENS_FN bool lens_certified(const LensCoeffs& c, float xu, float yu, float xd, float yd, float fx, float fy) {
    float xr, yr;
    lens_distort(c, xu, yu, xr, yr);
    return fabsf((xr - xd) * fx) <= kLensCertificate && fabsf((yr - yd) * fy) <= kLensCertificate;
}

// Step 5's window: a position that passes lies in (-3, size + 2), so floorf of it, the taps' offsets added, fits an int; a NaN fails.  Every filter's taps of a
// position outside the window lie outside the source (Catmull-Rom reaches floorf(s) - 1 .. floorf(s) + 2).
DSRT_LENS_FN bool lens_in_window(float s, int size) { return s > -3.0f && s < (float)size + 2.0f; }

// Step 6: Catmull-Rom's four weights for the taps floorf(s) - 1 .. floorf(s) + 2, t = s - floorf(s).
DSRT_LENS_FN void lens_cubic_weights(float t, float (&w)[4]) {
    w[0] = (((-0.5f * t) + 1.0f) * t - 0.5f) * t;
    w[1] = (((1.5f * t) - 2.5f) * t) * t + 1.0f;
    w[2] = (((-1.5f * t) + 2.0f) * t + 0.5f) * t;
    w[3] = (((0.5f * t) - 0.5f) * t) * t;
}

// Step 7: the gain at the undistorted position.
DSRT_LENS_FN float lens_vignette(float v1, float v2, float v3, int cos4, float xu, float yu) {
    const float ru2 = xu * xu + yu * yu;
    float g = 1.0f + ru2 * (v1 + ru2 * (v2 + ru2 * v3));
    if (cos4) {
        const float q = 1.0f + ru2;
        g = g / (q * q);
    }
    return fmaxf(g, 0.0f);
}

}  // namespace dsrt
