// sensor_kernel.hip -- the detector model of include/dsrt.h (SENSOR MODEL): one kernel, blur and detector in one pass over the linear frame.
//
//   dsrt_sensor_kernel<C, HAS_PSF>   C = 3 (colour: the three input channels are the planes) or 1 (mono: the luminance of the input pixel, taken before the blur).
//
//   HAS_PSF = true    a workgroup of 256 threads owns a tile of 64 x 16 output pixels and stages the tile plus a halo of r = (psf_size - 1) / 2 pixels of every plane
//                     in LDS: (64 + 2r) x (16 + 2r) floats per plane, 18 KB at r = 16, 54 KB for three planes.  A wave owns 64 columns x 4 rows of the tile, a lane
//                     one column of them: its four pixels of a plane read the same 2r + 4 rows of that LDS column, so the lane walks those rows ONCE (tile row t
//                     outer, kx inner), reads each LDS dword once and feeds it to the up to four pixels whose window holds it -- pixel j takes it as its tap
//                     ky = t - j - r.  Each pixel keeps its own accumulator per plane and meets its taps with ky ascending and, within a row, kx ascending: the
//                     header's order, nothing reassociated.  Consecutive lanes read consecutive LDS dwords (conflict-free ds_read_b32); the tap index is the same
//                     for the whole wave, so the taps come through scalar loads.
//                     OUTSIDE THE IMAGE the tile holds +0.0f, and the inner loop has no branch: of the two ways the header allows, this is the sentinel, and the
//                     sentinel needs no test.  A skipped tap and s + w * (+0.0f) give the same bits: w is finite and >= 0 (the entry point refuses any other tap),
//                     so the product is +0.0f, and the accumulator is never -0.0f (it starts at +0.0f, and a sum is -0.0f only when both terms are), so adding
//                     +0.0f returns it unchanged.  What lies outside is the zero the kernel wrote, never an input value, so a non-finite input cannot leak in.
//   HAS_PSF = false   no tile, no LDS: one pixel per lane, s = +0.0f + 1.0f * c, which is psf_size 1 with the tap 1.0f.
//
// The detector (the header's steps 3 to 6) runs per pixel and plane on the finished s; it is skipped altogether when only d_signal is asked for.  A draw whose
// coefficient is zero is not generated (the three conditions are kernel arguments: uniform branches).  Draws are philox4x32_10_block of device_math.h, unchanged.
//
// Every index is bounded where it is formed: a pixel is loaded into the tile only when 0 <= gx < W and 0 <= gy < H, a tile entry is read only at
// 0 <= row < 16 + 2r and 0 <= column < 64 + 2r (lane + kx + r, kx + r <= 2r), a tap only at 0 <= index < psf_size^2, and a pixel is written only when x < W and
// y < H.  W * H < 2^31 (the entry point refuses more), so pixel numbers fit 32 bits and element offsets are formed in size_t.
// There is no reference counterpart: the reference stops at an 8-bit PPM.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, no fast-math -- IEEE division, sqrtf and the absence of contraction are the contract.
#include "../../include/dsrt.h"
#include "device_math.h"
#include "launchers.h"

namespace dsrt {

namespace {

constexpr int kTileW = 64, kTileH = 16, kRows = 4;             // a workgroup's pixels; rows per lane (kTileH = 4 waves x kRows)
constexpr float kInvSigma = 0x1.3988e2p-16f;                   // the fp32 value nearest 1 / sqrt(2863311530) (include/dsrt.h, SENSOR MODEL, step 3)

__device__ __forceinline__ float sn_input(const float* __restrict__ in, size_t pixel, int k, bool mono) {
    const float* p = in + pixel * 3;
    if (!mono) return p[k];
    return (0.2126f * p[0] + 0.7152f * p[1]) + 0.0722f * p[2];
}

// One Gaussian-like draw: the Irwin-Hall sum of the eight 16-bit halves of one Philox block, centred and scaled to unit variance.
__device__ __forceinline__ float sn_draw(const SensorArgs& a, uint32_t pixel, uint32_t plane, uint32_t kind) {
    uint32_t o0, o1, o2, o3;
    philox4x32_10_block(a.seed_lo, a.seed_hi, pixel, plane + 4u * kind, kind == 0u ? a.frame : 0u, 0x53454E53u, o0, o1, o2, o3);
    const uint32_t S = ((o0 & 0xFFFFu) + (o0 >> 16)) + ((o1 & 0xFFFFu) + (o1 >> 16)) + ((o2 & 0xFFFFu) + (o2 >> 16)) + ((o3 & 0xFFFFu) + (o3 >> 16));
    return ((float)S - 262140.0f) * kInvSigma;
}

// Steps 3 to 6 for plane k of `pixel`, whose blurred signal is s: the outputs that are asked for.
template <int C>
__device__ __forceinline__ void sn_detect(const SensorArgs& a, uint32_t pixel, int k, float s) {
    const size_t at = (size_t)pixel * C + (size_t)k;
    if (a.out_signal) a.out_signal[at] = s;
    if (!a.out_dn && !a.out_rgb8) return;
    const float z1 = a.prnu != 0.0f ? sn_draw(a, pixel, (uint32_t)k, 1u) : 0.0f;
    const float z2 = a.dsnu_e != 0.0f ? sn_draw(a, pixel, (uint32_t)k, 2u) : 0.0f;
    const float z0 = a.noise != 0 ? sn_draw(a, pixel, (uint32_t)k, 0u) : 0.0f;
    float e = s * a.gain_e;
    e = e * (1.0f + a.prnu * z1);
    const float d = fmaxf(a.dark_e + a.dsnu_e * z2, 0.0f);
    const float m = fmaxf(e, 0.0f) + d;
    const float sg = sqrtf(m + a.read_e * a.read_e);
    const float q = fminf(m + sg * z0, a.full_well_e);
    const float v = floorf((q / a.e_per_dn + a.offset_dn) + 0.5f);
    const uint32_t top = (1u << a.bits) - 1u;
    const uint32_t dn = !(v >= 0.0f) ? 0u : (v > (float)top ? top : (uint32_t)v);
    if (a.out_dn) a.out_dn[at] = (uint16_t)dn;
    if (a.out_rgb8) {
        const uint8_t b = (uint8_t)(dn >> (a.bits - 8));
        uint8_t* o = a.out_rgb8 + (size_t)pixel * 3;
        if (C == 3) o[k] = b;
        else { o[0] = b; o[1] = b; o[2] = b; }
    }
}

// The taps of tile row t for the lane's kRows pixels: pixel j takes the row as ky = t - j - r, tap row (r - ky) = 2r - t + j.  ALL: every pixel's window holds
// the row (kRows - 1 <= t <= 2r), so no test; otherwise `take` says which do (wave-uniform either way).
template <int C, bool ALL>
__device__ __forceinline__ void sn_tile_row(const float* __restrict__ psf, int n, int r, int t, const float* row, int plane_stride, float (&s)[C][kRows]) {
    bool take[kRows];
    const float* taps[kRows];
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
        const int pr = 2 * r - t + j;                           // the tap row; inside [0, n) exactly when the window holds the tile row
        take[j] = ALL || (pr >= 0 && pr < n);
        taps[j] = psf + (take[j] ? pr : 0) * n + (n - 1);       // ... its LAST tap: kx = -r is tap column r - kx = 2r = n - 1, and the column falls as kx rises
    }
    // (unrolled by 4: left to itself the compiler unrolls the one-plane loop by 8 and spills scalar registers)
#pragma unroll 4
    for (int c = 0; c < n; ++c) {                               // c = kx + r
        float v[C];
#pragma unroll
        for (int k = 0; k < C; ++k) v[k] = row[k * plane_stride + c];
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            if (!take[j]) continue;
            const float w = taps[j][-c];
#pragma unroll
            for (int k = 0; k < C; ++k) s[k][j] = s[k][j] + w * v[k];
        }
    }
}

}  // namespace

template <int C, bool HAS_PSF>
__global__ __launch_bounds__(256) void dsrt_sensor_kernel(const SensorArgs a) {
    const bool mono = C == 1;
    if constexpr (!HAS_PSF) {
        const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
        if (i >= (size_t)a.W * (size_t)a.H) return;
#pragma unroll
        for (int k = 0; k < C; ++k) sn_detect<C>(a, (uint32_t)i, k, 0.0f + 1.0f * sn_input(a.in, i, k, mono));
    } else {
        extern __shared__ float tile[];
        const int n = a.psf_size, r = (n - 1) >> 1;
        const int tw = kTileW + 2 * r, th = kTileH + 2 * r, plane_stride = tw * th;
        const int tiles_x = (a.W + kTileW - 1) / kTileW;
        const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kTileW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kTileH;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        for (int ty = wave; ty < th; ty += 4) {
            const int gy = y0 - r + ty;
            for (int tx = lane; tx < tw; tx += 64) {
                const int gx = x0 - r + tx;
                const bool inside = gx >= 0 && gx < a.W && gy >= 0 && gy < a.H;
#pragma unroll
                for (int k = 0; k < C; ++k) tile[k * plane_stride + ty * tw + tx] = inside ? sn_input(a.in, (size_t)gy * (size_t)a.W + (size_t)gx, k, mono) : 0.0f;
            }
        }
        __syncthreads();
        float s[C][kRows];
#pragma unroll
        for (int k = 0; k < C; ++k)
#pragma unroll
            for (int j = 0; j < kRows; ++j) s[k][j] = 0.0f;
        const float* __restrict__ const psf = a.psf;
        const float* col = tile + (wave * kRows) * tw + lane;   // the lane's column at the first tile row its pixels read
        const int rows = 2 * r + kRows;                         // tile rows t = 0 .. 2r + kRows - 1
        for (int t = 0; t < rows; ++t) {
            if (t >= kRows - 1 && t <= 2 * r) sn_tile_row<C, true>(psf, n, r, t, col + t * tw, plane_stride, s);
            else sn_tile_row<C, false>(psf, n, r, t, col + t * tw, plane_stride, s);
        }
        const int x = x0 + lane;
        if (x >= a.W) return;
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int y = y0 + wave * kRows + j;
            if (y >= a.H) break;
            const uint32_t pixel = (uint32_t)y * (uint32_t)a.W + (uint32_t)x;
#pragma unroll
            for (int k = 0; k < C; ++k) sn_detect<C>(a, pixel, k, s[k][j]);
        }
    }
}

hipError_t launch_sensor(const SensorArgs& a, bool mono, hipStream_t stream) {
    if (!a.psf) {
        const dim3 grid((unsigned)(((size_t)a.W * (size_t)a.H + 255) / 256));
        if (mono) hipLaunchKernelGGL((dsrt_sensor_kernel<1, false>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((dsrt_sensor_kernel<3, false>), grid, dim3(256), 0, stream, a);
        return hipGetLastError();
    }
    const int r = (a.psf_size - 1) / 2;
    const size_t plane = (size_t)(kTileW + 2 * r) * (size_t)(kTileH + 2 * r) * sizeof(float);
    const dim3 grid((unsigned)((size_t)((a.W + kTileW - 1) / kTileW) * (size_t)((a.H + kTileH - 1) / kTileH)));
    if (mono) hipLaunchKernelGGL((dsrt_sensor_kernel<1, true>), grid, dim3(256), plane, stream, a);
    else hipLaunchKernelGGL((dsrt_sensor_kernel<3, true>), grid, dim3(256), 3 * plane, stream, a);
    return hipGetLastError();
}

}  // namespace dsrt
