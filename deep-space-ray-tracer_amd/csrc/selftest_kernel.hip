// selftest_kernel.hip -- small kernels beside the renderer: the tile de-interleave of a multi-GPU gather, the drop-in layer's content hash, and the self-test hooks
// that run device_math.h's functions on explicit inputs (math, devkat, philox): the default mode's deterministic sin / cos / pow, so compiled once.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (no fast-math: IEEE div/sqrt are part of the contract).
#include <rocrand/rocrand_kernel.h>

#include "device_math.h"
#include "launchers.h"

namespace dsrt {

// Tile-major shards -> image order, on the root after the gather.
__global__ void dsrt_deinterleave_kernel(const uint8_t* __restrict__ gathered, uint8_t* __restrict__ image, int W, int H, int tile, int tiles_x,
                                         int shard_count, size_t shard_stride_bytes) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)W * H) return;
    const int x = (int)(i % W), row = (int)(i / W);
    const int g = (row / tile) * tiles_x + (x / tile);
    const int rank = g % shard_count, k = g / shard_count;
    const size_t src = (size_t)rank * shard_stride_bytes + ((size_t)k * tile * tile + (size_t)(row % tile) * tile + (x % tile)) * 3;
    image[i * 3 + 0] = gathered[src + 0];
    image[i * 3 + 1] = gathered[src + 1];
    image[i * 3 + 2] = gathered[src + 2];
}

__global__ void dsrt_math_kernel(int fn, const float* __restrict__ x, float y, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = fn == 0 ? dsrt_sinf(x[i]) : (fn == 1 ? dsrt_cosf(x[i]) : dsrt_powf(x[i], y));
}

// Test hook (dsrt_selftest_devkat): the render kernel's own material / frame helpers of device_math.h on explicit inputs, 12 words in and
// 12 words out per case, so that they can be compared with known answers produced by the reference's host code (tests/golden/ref_matkat.json).
//   fn 0 reflect            in: v[3] n[3]                              out: r[3]
//   fn 1 refract            in: v[3] n[3] eta                          out: r[3]
//   fn 2 scatter_metal      in: dir[3] n[3] fuzz, LCG state (bits)     out: dir[3], went on (1.0 / 0.0), LCG state after (bits)
//   fn 3 scatter_dielectric in: dir[3] n[3] ref_idx, state, front face out: dir[3], -, LCG state after (bits)
//   fn 4 build_onb          in: n[3]                                   out: u[3] v[3] w[3]
//   fn 5 schlick            in: cosine, ratio                          out: reflectance
__global__ void dsrt_devkat_kernel(int fn, const float* __restrict__ in, float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* a = in + (size_t)i * 12;
    float* o = out + (size_t)i * 12;
    const F3 v = ld3(a), nn = ld3(a + 3);
    uint32_t rng = __float_as_uint(a[7]);
    if (fn == 0) { const F3 r = reflect(v, nn); o[0] = r.x; o[1] = r.y; o[2] = r.z; }
    else if (fn == 1) { const F3 r = refract(v, nn, a[6]); o[0] = r.x; o[1] = r.y; o[2] = r.z; }
    else if (fn == 2) { F3 d; const bool ok = scatter_metal(v, nn, a[6], rng, d); o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = ok ? 1.0f : 0.0f; o[4] = __uint_as_float(rng); }
    else if (fn == 3) { const F3 d = scatter_dielectric(v, nn, __float_as_uint(a[8]) != 0u, a[6], rng); o[0] = d.x; o[1] = d.y; o[2] = d.z; o[4] = __uint_as_float(rng); }
    else if (fn == 4) { F3 u, vv, w; build_onb(v, u, vv, w); o[0] = u.x; o[1] = u.y; o[2] = u.z; o[3] = vv.x; o[4] = vv.y; o[5] = vv.z; o[6] = w.x; o[7] = w.y; o[8] = w.z; }
    else { o[0] = schlick(a[0], a[1]); }
}

hipError_t launch_devkat(int fn, const float* in, float* out, int n, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_devkat_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, fn, in, out, n);
    return hipGetLastError();
}

// Test hook: the first n words of Philox sub-sequence `sub` from our stateless form and from rocRAND's own device engine.
__global__ void dsrt_philox_kernel(unsigned long long seed, unsigned long long sub, int n, uint32_t* __restrict__ ours, uint32_t* __restrict__ theirs) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    rocrand_state_philox4x32_10 st;
    rocrand_init(seed, sub, 0, &st);
    for (int i = 0; i < n; ++i) {
        ours[i] = philox4x32_10_word((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)i >> 2, 0u, (uint32_t)sub, (uint32_t)(sub >> 32), (uint32_t)i & 3u);
        theirs[i] = rocrand(&st);
    }
}

hipError_t launch_philox(unsigned long long seed, unsigned long long sub, int n, uint32_t* ours, uint32_t* theirs, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_philox_kernel, dim3(1), dim3(64), 0, stream, seed, sub, n, ours, theirs);
    return hipGetLastError();
}

hipError_t launch_deinterleave(const uint8_t* gathered, uint8_t* image, int W, int H, int tile, int tiles_x, int shard_count,
                               size_t shard_stride_bytes, hipStream_t stream) {
    const size_t n = (size_t)W * H;
    hipLaunchKernelGGL(dsrt_deinterleave_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, gathered, image, W, H, tile, tiles_x,
                       shard_count, shard_stride_bytes);
    return hipGetLastError();
}

// 128-bit position-dependent content hash of a word array (the drop-in layer's "same scene as last frame?" test, api_dropin.hip):
// two independent 64-bit mixes of (word, index, salt), summed -- addition commutes, so blocks may finish in any order.
__global__ void __launch_bounds__(256) dsrt_content_hash_kernel(const uint32_t* __restrict__ words, size_t n, uint64_t salt, uint64_t* __restrict__ out2) {
    uint64_t a = 0, b = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t x = ((uint64_t)words[i] << 32 | (uint64_t)(uint32_t)i) ^ salt ^ ((uint64_t)(i >> 32) * 0xD6E8FEB86659FD93ull);
        x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
        a += x;
        uint64_t y = x ^ 0xA0761D6478BD642Full;
        y ^= y >> 29; y *= 0xBF58476D1CE4E5B9ull; y ^= y >> 32;
        b += y * 0x94D049BB133111EBull;
    }
    for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
    if ((threadIdx.x & 63) == 0) { atomicAdd((unsigned long long*)&out2[0], (unsigned long long)a); atomicAdd((unsigned long long*)&out2[1], (unsigned long long)b); }
}

hipError_t launch_content_hash(const uint32_t* words, size_t n_words, uint64_t salt, uint64_t* d_hash2, hipStream_t stream) {
    if (!n_words) return hipSuccess;
    const size_t want = (n_words + 255) / 256;
    hipLaunchKernelGGL(dsrt_content_hash_kernel, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, stream, words, n_words, salt, d_hash2);
    return hipGetLastError();
}

hipError_t launch_math(int fn, const float* x, float y, float* out, int n, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_math_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, fn, x, y, out, n);
    return hipGetLastError();
}

}  // namespace dsrt
