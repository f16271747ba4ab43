// sample_set_kernel.hip -- the small kernels around the integer sums of rng_mode 1 (include/dsrt.h, SAMPLE SETS and ADAPTIVE SAMPLING): the lists of active pixels of
// a masked accumulate launch, the per-pixel sample counts, the convergence test, and the resolve of sums to an image.  The arithmetic on the sums is
// pixel_arith.h's; the resolve is templated over where powf comes from (DsrtRenderDesc.math_mode), so nothing here needs render_kernel.hip's second compilation.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (no fast-math: IEEE div/sqrt are part of the contract).
#include "launchers.h"
#include "pixel_arith.h"

namespace dsrt {

// The lists of a masked accumulate launch (path_machine.h, LISTED), built behind the pre-pass on its stream in three small kernels: one wave per 8x8 block of every
// tile in the order, heavy part and light part, counts its active pixels (mask byte != 0) with a ballot; one workgroup turns the counts into offsets (a prefix sum
// along the order) and writes the two lengths, which ST_FETCH reads afterwards -- no readback; the waves of the first kernel's shape then write their pixels at
// offset + rank in the ballot.  So a list is in the tile order itself, block by block and pixel by pixel as the tile FETCH walks a tile: with every pixel active an
// item number means the pixel it means in an unmasked launch, and the costliest tiles' pixels come first whatever order the waves ran in.  (A first form appended
// with one atomicAdd per wave on the length word: the blocks then arrive in the order the atomics were served.)  The heavy list has room for every pixel of the
// heavy tiles, the light list starts right behind that, and the per-wave counts lie behind both.  The counting threads, one per pixel of the image (culled tiles
// included: the rule does not depend on culling), also add `count` to n[] where the mask is set.
struct ListWave { uint32_t pos, x, row; bool live, active; unsigned long long votes; };
__device__ __forceinline__ ListWave list_wave(uint32_t wave_id, uint32_t lane, int W, int H, int tile, int tiles_x, const uint32_t* __restrict__ order,
                                              const uint32_t* __restrict__ sched, const uint8_t* __restrict__ mask) {
    const uint32_t per_row = (uint32_t)tile >> 3, blocks_per_tile = per_row * per_row;
    ListWave w;
    w.pos = wave_id / blocks_per_tile;                                                    // place in the tile order
    const uint32_t sub = wave_id % blocks_per_tile;                                       // 8x8 block of that tile
    w.live = w.pos < sched[1];                                                            // (wave-uniform)
    w.x = w.row = 0; w.active = false;
    if (w.live) {
        const uint32_t k = order ? order[w.pos] : w.pos;
        w.x = (k % (uint32_t)tiles_x) * (uint32_t)tile + (sub % per_row) * 8u + (lane & 7u);
        w.row = (k / (uint32_t)tiles_x) * (uint32_t)tile + (sub / per_row) * 8u + (lane >> 3);
        w.active = w.x < (uint32_t)W && w.row < (uint32_t)H && mask[(size_t)w.row * (uint32_t)W + w.x] != 0;
    }
    w.votes = wave_ballot(w.active);
    return w;
}

__global__ void __launch_bounds__(256) dsrt_pixel_count_kernel(int W, int H, int tile, int tiles_x, const uint32_t* __restrict__ order, const uint32_t* __restrict__ sched,
                                                               const uint8_t* __restrict__ mask, uint32_t* __restrict__ offs, uint32_t* __restrict__ n, uint32_t count) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (n && gid < (uint32_t)W * (uint32_t)H && mask[gid]) n[gid] += count;
    const ListWave w = list_wave(gid >> 6, threadIdx.x & 63u, W, H, tile, tiles_x, order, sched, mask);
    if (w.live && (threadIdx.x & 63u) == 0u) offs[gid >> 6] = (uint32_t)__popcll(w.votes);
}

// offs[0 .. n_live * blocks_per_tile): counts in, their exclusive prefix sums out; list_len = the sum over the heavy tiles' blocks, the sum over the rest.
__global__ void __launch_bounds__(1024) dsrt_pixel_scan_kernel(int tile, const uint32_t* __restrict__ sched, uint32_t* __restrict__ offs, uint32_t* __restrict__ list_len) {
    __shared__ uint32_t part[1024], heavy_total;
    const uint32_t blocks_per_tile = (uint32_t)((tile >> 3) * (tile >> 3));
    const uint32_t total = sched[1] * blocks_per_tile, boundary = sched[0] * blocks_per_tile;
    const uint32_t each = (total + 1023u) / 1024u, lo = min(total, threadIdx.x * each), hi = min(total, lo + each);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += offs[i];
    part[threadIdx.x] = sum;
    if (threadIdx.x == 0) heavy_total = 0;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {                                            // inclusive scan of the 1024 partial sums
        const uint32_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t i = lo; i < hi; ++i) {
        if (i == boundary) heavy_total = run;
        const uint32_t c = offs[i];
        offs[i] = run;
        run += c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t all = part[1023], h = boundary >= total ? all : heavy_total;
        list_len[0] = h;
        list_len[1] = all - h;
    }
}

__global__ void __launch_bounds__(256) dsrt_pixel_list_kernel(int W, int H, int tile, int tiles_x, const uint32_t* __restrict__ order, const uint32_t* __restrict__ sched,
                                                              const uint8_t* __restrict__ mask, const uint32_t* __restrict__ offs, uint32_t* __restrict__ list,
                                                              const uint32_t* __restrict__ list_len) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    const ListWave w = list_wave(gid >> 6, threadIdx.x & 63u, W, H, tile, tiles_x, order, sched, mask);
    if (w.votes == 0ull) return;                                                          // (a wave past the live tiles has none)
    const uint32_t n_heavy = sched[0], tt = (uint32_t)(tile * tile);
    // offsets run on through both parts: the light list's own start is the heavy list's length, and its place is behind the heavy tiles' pixels
    const uint32_t base = w.pos < n_heavy ? offs[gid >> 6] : n_heavy * tt + (offs[gid >> 6] - list_len[0]);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(w.votes >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)w.votes, 0u));
    if (w.active) list[base + rank] = w.x | (w.row << 16);
}

// `list`: local_tiles * tile^2 entries for the two lists and, behind them, one word per 8x8 block of every tile for the counts and offsets.
hipError_t launch_pixel_list(const FrameParams& P, const uint32_t* order, const uint32_t* sched, const uint8_t* mask, uint32_t* list, uint32_t* list_len,
                             uint32_t* n, uint32_t count, hipStream_t stream) {
    const size_t threads = (size_t)P.local_tiles * (size_t)(P.tile * P.tile);            // one per pixel of every tile: at least width * height
    const dim3 grid((unsigned)((threads + 255) / 256));
    uint32_t* offs = list + threads;
    hipLaunchKernelGGL(dsrt_pixel_count_kernel, grid, dim3(256), 0, stream, P.width, P.height, P.tile, P.tiles_x, order, sched, mask, offs, n, count);
    hipLaunchKernelGGL(dsrt_pixel_scan_kernel, dim3(1), dim3(1024), 0, stream, P.tile, sched, offs, list_len);
    hipLaunchKernelGGL(dsrt_pixel_list_kernel, grid, dim3(256), 0, stream, P.width, P.height, P.tile, P.tiles_x, order, (const uint32_t*)sched, mask,
                       (const uint32_t*)offs, list, (const uint32_t*)list_len);
    return hipGetLastError();
}

// n[] += count for every pixel: what an unmasked pass of dsrt_render_adaptive adds to the sample counts.
__global__ void dsrt_add_count_kernel(uint32_t* __restrict__ n, uint32_t count, size_t n_pixels) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_pixels) n[i] += count;
}

hipError_t launch_add_count(uint32_t* n, uint32_t count, size_t n_pixels, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_add_count_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, n, count, n_pixels);
    return hipGetLastError();
}

// The convergence test of adaptive sampling (include/dsrt.h, ADAPTIVE SAMPLING): in double, in exactly the order the header writes down -- conversions, one
// multiplication by a power of two, and correctly rounded + - * / only (no fused operations: -ffp-contract=off; no sqrt) -- so that a CPU reproduces every byte.
__global__ void __launch_bounds__(256) dsrt_select_unconverged_kernel(const unsigned long long* __restrict__ sums, const unsigned long long* __restrict__ sums_sq,
                                                                      const uint32_t* __restrict__ counts, size_t n_pixels, float rel_tol, float floor_, uint32_t n_min,
                                                                      uint32_t n_max, uint8_t* __restrict__ mask, uint32_t* __restrict__ n_active) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool active = false;
    if (i < n_pixels) {
        const uint32_t cnt = counts[i];
        bool converged = cnt >= 2u;
        if (converged) {
            const double n = (double)cnt;
            for (int ch = 0; ch < 3; ++ch) {
                double s;
                const double v = sum_variance(sums[i * 3 + ch], sums_sq[i * 3 + ch], n, s);
                const double vm = v / n, m = s / n;
                const double r = m > (double)floor_ ? m : (double)floor_;
                const double lim = (double)rel_tol * r;
                converged = converged && vm <= lim * lim;
            }
        }
        active = cnt < n_max && (cnt < n_min || !converged);
        mask[i] = active ? 1 : 0;
    }
    if (n_active) {
        const unsigned long long votes = wave_ballot(active);
        if ((threadIdx.x & 63u) == 0u && votes != 0ull) atomicAdd(n_active, (uint32_t)__popcll(votes));
    }
}

hipError_t launch_select_unconverged(const unsigned long long* sums, const unsigned long long* sums_sq, const uint32_t* counts, size_t n_pixels, float rel_tol, float floor_,
                                     uint32_t n_min, uint32_t n_max, uint8_t* mask, uint32_t* n_active, hipStream_t stream) {
    if (!n_pixels) return hipSuccess;
    hipLaunchKernelGGL(dsrt_select_unconverged_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, sums, sums_sq, counts, n_pixels, rel_tol, floor_,
                       n_min, n_max, mask, n_active);
    return hipGetLastError();
}

// The resolve of rng_mode 1: a pixel's samples were summed as integers in units of 2^-20 (path_machine.h, end_sample); here the mean over the samples summed, the
// tone map and the 8-bit store, and with sums_sq (dsrt_resolve_accumulated, include/dsrt.h) the variance of the mean -- pixel_arith.h's arithmetic throughout.
// One body behind two kernels: n is samples_done for every pixel, or with PER_PIXEL_COUNTS (dsrt_resolve_accumulated_counts: adaptive sampling) the pixel's own
// counts[i].  Pixels nobody sampled hold zero sums: black; with PER_PIXEL_COUNTS n == 0 is zero bytes and +0.0f whatever the sums, and n == 1 has variance +0.0f.
template <bool DEVICE_LIBM, bool PER_PIXEL_COUNTS>
__device__ __forceinline__ void resolve_pixel(const unsigned long long* __restrict__ sums, int samples_done, const uint32_t* __restrict__ counts, float inv_gamma,
                                              size_t n_pixels, uint8_t* __restrict__ out_rgb8, float* __restrict__ out_f32,
                                              const unsigned long long* __restrict__ sums_sq, float* __restrict__ out_var) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_pixels) return;
    uint32_t cnt = 0;
    if constexpr (PER_PIXEL_COUNTS) cnt = counts[i];
    const double n = PER_PIXEL_COUNTS ? (double)cnt : (double)samples_done;
    if (out_var) {
        for (int ch = 0; ch < 3; ++ch) {
            float var = 0.0f;
            if (!PER_PIXEL_COUNTS || cnt >= 2u) {
                double s;
                var = (float)(sum_variance(sums[i * 3 + ch], sums_sq[i * 3 + ch], n, s) / n);
            }
            out_var[i * 3 + ch] = var;
        }
    }
    if (!out_rgb8 && !out_f32) return;
    F3 col = mk(0, 0, 0);
    if (!PER_PIXEL_COUNTS || cnt) col = tone_map<DEVICE_LIBM>(mk(sum_mean(sums[i * 3 + 0], n), sum_mean(sums[i * 3 + 1], n), sum_mean(sums[i * 3 + 2], n)), inv_gamma);
    if (out_rgb8) store_rgb8(out_rgb8, i * 3, col);
    if (out_f32) { out_f32[i * 3 + 0] = col.x; out_f32[i * 3 + 1] = col.y; out_f32[i * 3 + 2] = col.z; }
}

template <bool DEVICE_LIBM>
__global__ void dsrt_resolve_kernel(const unsigned long long* __restrict__ sums, int samples_done, float inv_gamma, size_t n_pixels,
                                    uint8_t* __restrict__ out_rgb8, float* __restrict__ out_f32,
                                    const unsigned long long* __restrict__ sums_sq, float* __restrict__ out_var) {
    resolve_pixel<DEVICE_LIBM, false>(sums, samples_done, nullptr, inv_gamma, n_pixels, out_rgb8, out_f32, sums_sq, out_var);
}

template <bool DEVICE_LIBM>
__global__ void dsrt_resolve_counts_kernel(const unsigned long long* __restrict__ sums, const uint32_t* __restrict__ counts, float inv_gamma, size_t n_pixels,
                                           uint8_t* __restrict__ out_rgb8, float* __restrict__ out_f32,
                                           const unsigned long long* __restrict__ sums_sq, float* __restrict__ out_var) {
    resolve_pixel<DEVICE_LIBM, true>(sums, 0, counts, inv_gamma, n_pixels, out_rgb8, out_f32, sums_sq, out_var);
}

hipError_t launch_resolve(const unsigned long long* sums, int samples_done, float inv_gamma, bool device_libm, size_t n_pixels, uint8_t* out_rgb8, float* out_f32,
                          const unsigned long long* sums_sq, float* out_var, hipStream_t stream) {
    if (!n_pixels) return hipSuccess;
    const dim3 grid((unsigned)((n_pixels + 255) / 256)), block(256);
    if (device_libm) hipLaunchKernelGGL(dsrt_resolve_kernel<true>, grid, block, 0, stream, sums, samples_done, inv_gamma, n_pixels, out_rgb8, out_f32, sums_sq, out_var);
    else hipLaunchKernelGGL(dsrt_resolve_kernel<false>, grid, block, 0, stream, sums, samples_done, inv_gamma, n_pixels, out_rgb8, out_f32, sums_sq, out_var);
    return hipGetLastError();
}

hipError_t launch_resolve_counts(const unsigned long long* sums, const uint32_t* counts, float inv_gamma, bool device_libm, size_t n_pixels, uint8_t* out_rgb8,
                                 float* out_f32, const unsigned long long* sums_sq, float* out_var, hipStream_t stream) {
    if (!n_pixels) return hipSuccess;
    const dim3 grid((unsigned)((n_pixels + 255) / 256)), block(256);
    if (device_libm) hipLaunchKernelGGL(dsrt_resolve_counts_kernel<true>, grid, block, 0, stream, sums, counts, inv_gamma, n_pixels, out_rgb8, out_f32, sums_sq, out_var);
    else hipLaunchKernelGGL(dsrt_resolve_counts_kernel<false>, grid, block, 0, stream, sums, counts, inv_gamma, n_pixels, out_rgb8, out_f32, sums_sq, out_var);
    return hipGetLastError();
}

}  // namespace dsrt
