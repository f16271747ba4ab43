// lens_kernel.hip -- the lens model of include/dsrt.h (LENS MODEL): one kernel, one lane per OUTPUT pixel -- normalise, invert the distortion, certify, gather the
// taps from the pinhole frame, apply the flat field.
//
//   dsrt_lens_kernel<C, FILTER>   C = 1 .. 4 interleaved 32-bit words per pixel; FILTER 0 nearest (words copied), 1 bilinear, 2 Catmull-Rom.
//
// A DIRECT GATHER.  A workgroup of 256 threads owns 64 x 4 output pixels: a wave one row of 64, a lane one pixel.  The twelve inverse steps run in registers (the
// arithmetic is lens_math.h's, which the host compiles too); the taps are plain vector loads.  The distortion is smooth, so the 64 lanes of a wave read a run of
// neighbouring source texels per tap row (at magnification m about 64 / m of them), the four waves of a workgroup neighbouring rows, and the 4 x 4 footprints of
// neighbouring lanes overlap: what is fetched more than once comes from L1 and L2, and the source frame as a whole (100 MB at 4K colour) fits the Infinity Cache.
// The loop count is fixed and the certificate is a select, so control flow is wave-uniform up to the taps; there a lane whose pixel has no source skips its loads.
//
// Every index is bounded where it is formed: a lane works only on x < W and y < H; a source position is turned into an integer only after lens_in_window (floats,
// a NaN fails) has put it inside (-3, size + 2); a texel is read only when 0 <= qx < src_width and 0 <= qy < src_height (tap by tap), at the element offset
// ((size_t)qy * src_width + qx) * C + k; the outputs are written at the lane's own pixel, by plain vector stores.  Both frames have fewer than 2^31 pixels (the
// entry point refuses more).
// There is no reference counterpart: the reference's camera is a pinhole.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, no fast-math -- IEEE division and the absence of contraction are the contract.
#include "../../include/dsrt.h"
#include "launchers.h"
#include "lens_math.h"

namespace dsrt {

namespace {

constexpr int kLensTileW = 64, kLensTileH = 4;                 // a workgroup's output pixels: one wave per row

__device__ __forceinline__ bool lens_inside(const LensArgs& a, int qx, int qy) { return qx >= 0 && qx < a.src_w && qy >= 0 && qy < a.src_h; }

}  // namespace

template <int C, int FILTER>
__global__ __launch_bounds__(256) void dsrt_lens_kernel(const LensArgs a) {
    const int tiles_x = (a.W + kLensTileW - 1) / kLensTileW;
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * kLensTileW + (int)(threadIdx.x & 63u);
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * kLensTileH + (int)(threadIdx.x >> 6);
    if (x >= a.W || y >= a.H) return;
    const size_t pixel = (size_t)y * (size_t)a.W + (size_t)x;

    // steps 1 to 5
    const float xd = ((float)x - a.cx) / a.fx, yd = ((float)y - a.cy) / a.fy;
    float xu, yu;
    lens_undistort(a.c, xd, yd, xu, yu);
    const bool inverted = lens_certified(a.c, xu, yu, xd, yd, a.fx, a.fy);
    const float sx = xu * a.src_fx + a.src_cx, sy = yu * a.src_fy + a.src_cy;
    const bool taps = inverted && lens_in_window(sx, a.src_w) && lens_in_window(sy, a.src_h);

    // steps 6 and 7
    constexpr int N = FILTER == DSRT_LENS_NEAREST ? 1 : (FILTER == DSRT_LENS_BILINEAR ? 2 : 4);
    int n_inside = 0;
    uint32_t word[C];
    if constexpr (FILTER == DSRT_LENS_NEAREST) {
#pragma unroll
        for (int k = 0; k < C; ++k) word[k] = a.fill_bits;
        if (taps) {
            const int qx = (int)floorf(sx + 0.5f), qy = (int)floorf(sy + 0.5f);
            if (lens_inside(a, qx, qy)) {
                const uint32_t* __restrict__ s = a.src + ((size_t)qy * (size_t)a.src_w + (size_t)qx) * C;
#pragma unroll
                for (int k = 0; k < C; ++k) word[k] = s[k];
                n_inside = 1;
            }
        }
    } else {
        float acc[C];
#pragma unroll
        for (int k = 0; k < C; ++k) acc[k] = 0.0f;
        if (taps) {
            const float fx0 = floorf(sx), fy0 = floorf(sy);
            const float tx = sx - fx0, ty = sy - fy0;
            float wx[N], wy[N];
            if constexpr (FILTER == DSRT_LENS_BILINEAR) {
                wx[0] = 1.0f - tx; wx[1] = tx;
                wy[0] = 1.0f - ty; wy[1] = ty;
            } else {
                lens_cubic_weights(tx, wx);
                lens_cubic_weights(ty, wy);
            }
            const int x0 = (int)fx0 - (N == 4 ? 1 : 0), y0 = (int)fy0 - (N == 4 ? 1 : 0);
            const float* __restrict__ const src = (const float*)a.src;
#pragma unroll
            for (int j = 0; j < N; ++j) {
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    if (!lens_inside(a, x0 + i, y0 + j)) continue;
                    const float* s = src + ((size_t)(y0 + j) * (size_t)a.src_w + (size_t)(x0 + i)) * C;
                    const float w = wy[j] * wx[i];
#pragma unroll
                    for (int k = 0; k < C; ++k) acc[k] = acc[k] + w * s[k];
                    ++n_inside;
                }
            }
        }
        if (inverted) {
            const float g = lens_vignette(a.v1, a.v2, a.v3, a.cos4, xu, yu);
#pragma unroll
            for (int k = 0; k < C; ++k) {
                float o = acc[k] * g;
                if (a.clamp_zero) o = fmaxf(o, 0.0f);
                word[k] = __float_as_uint(o);
            }
        } else {
#pragma unroll
            for (int k = 0; k < C; ++k) word[k] = 0u;
        }
    }

    // step 8
    if (a.out_image) {
        uint32_t* o = a.out_image + pixel * C;
#pragma unroll
        for (int k = 0; k < C; ++k) o[k] = word[k];
    }
    if (a.out_src_xy) {
        a.out_src_xy[pixel * 2] = inverted ? sx : 0.0f;
        a.out_src_xy[pixel * 2 + 1] = inverted ? sy : 0.0f;
    }
    if (a.out_status)
        a.out_status[pixel] = (uint8_t)((inverted ? DSRT_LENS_INVERTED : 0u) | (n_inside > 0 ? DSRT_LENS_ANY_TAP : 0u) | (n_inside == N * N ? DSRT_LENS_ALL_TAPS : 0u));
}

namespace {

template <int C>
hipError_t launch_lens_c(const LensArgs& a, int filter, dim3 grid, hipStream_t stream) {
    if (filter == DSRT_LENS_NEAREST) hipLaunchKernelGGL((dsrt_lens_kernel<C, DSRT_LENS_NEAREST>), grid, dim3(256), 0, stream, a);
    else if (filter == DSRT_LENS_BILINEAR) hipLaunchKernelGGL((dsrt_lens_kernel<C, DSRT_LENS_BILINEAR>), grid, dim3(256), 0, stream, a);
    else if (filter == DSRT_LENS_CUBIC) hipLaunchKernelGGL((dsrt_lens_kernel<C, DSRT_LENS_CUBIC>), grid, dim3(256), 0, stream, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

hipError_t launch_lens(const LensArgs& a, int channels, int filter, hipStream_t stream) {
    const size_t tiles = (size_t)((a.W + kLensTileW - 1) / kLensTileW) * (size_t)((a.H + kLensTileH - 1) / kLensTileH);
    const dim3 grid((unsigned)tiles);
    switch (channels) {
        case 1: return launch_lens_c<1>(a, filter, grid, stream);
        case 2: return launch_lens_c<2>(a, filter, grid, stream);
        case 3: return launch_lens_c<3>(a, filter, grid, stream);
        case 4: return launch_lens_c<4>(a, filter, grid, stream);
        default: return hipErrorInvalidValue;                   // a kernel that is missing is an error, never a fall-back
    }
}

}  // namespace dsrt
