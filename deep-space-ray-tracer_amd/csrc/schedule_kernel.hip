// schedule_kernel.hip -- the scheduling pre-pass of the render kernels (render_kernel.hip): the cost of every screen tile, the order tiles are handed out in, its
// refinement by a probe launch's measured work, and the table of a batch launch.  Scheduling only: none of it changes a pixel's value, or depends on where
// sinf / cosf / powf come from (compiled once).  tests/_schedule_model.py is the CPU model of the four kernels.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (no fast-math: IEEE div/sqrt are part of the contract).
#include "device_math.h"
#include "launchers.h"

namespace dsrt {

// Fills the count fields of the batch table (entries f and frames + f belong to frame f) from the sched words every frame's pre-pass
// wrote (sched_stride apart), and the running item totals.
__global__ void dsrt_batch_table_kernel(BatchFrame* __restrict__ table, const uint32_t* __restrict__ sched, uint32_t sched_stride, uint32_t frames,
                                        uint32_t tt, int rng_mode, int spp, int light_chunk_len, uint32_t* __restrict__ total_items) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    unsigned long long acc = 0;
    const uint32_t light_slices = rng_mode == 1 ? (uint32_t)((spp + light_chunk_len - 1) / light_chunk_len) : 1u;
    for (uint32_t e = 0; e < 2u * frames; ++e) {
        const uint32_t f = e < frames ? e : e - frames;
        const uint32_t* s = sched + (size_t)f * sched_stride;
        const uint32_t n_heavy = s[0], n_live = s[1];
        const uint32_t top = n_heavy ? (n_heavy >> 3 ? n_heavy >> 3 : 1u) : 0u;           // the first eighth of the heavy tiles, at least one
        BatchFrame& b = table[e];
        if (e < frames) { b.n_heavy = top; b.n_live = top; }
        else { b.n_heavy = n_heavy - top; b.n_live = n_live - top; b.order_base += top; }
        b.slices = rng_mode == 1 ? s[3] : 1u; b.chunk_len = rng_mode == 1 ? s[4] : (uint32_t)spp;
        acc += (unsigned long long)b.n_heavy * tt * b.slices + (unsigned long long)(b.n_live - b.n_heavy) * tt * light_slices;
        b.item_end = acc > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)acc;           // (the host bounds frames x pixels x 16 below 2^32)
    }
    *total_items = acc > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)acc;
}

// ---------------------------------------------------------------------------------------------------------------
// Scheduling pre-pass: how expensive is each screen tile?  One wave per 8x8 pixel block traces the un-jittered centre
// ray of every pixel with an any-hit walk; the tile's cost is the number of pixels that see geometry.  The render
// kernel then hands tiles out costliest first, so the pixels that are 1000-sample serial chains start early and the
// end of the frame is filled with background pixels instead of a long tail.  This changes only the ORDER in which
// pixels are rendered, never a pixel's value (each pixel depends on nothing but its own coordinates and the scene).
//
// Empty tiles.  With `cull` set, a block whose sample footprint cannot reach the root box is left out of the order
// altogether and its pixels keep the zeros the output was cleared to.  That is exact, not approximate: every sample of such
// a pixel fails the root test of bvh_hit_closest (:394-410), ray_color returns black (:744-747), the sum is 0 and the tone
// map of 0 is byte 0 -- whatever the pixel's random numbers were, and no other pixel reads them.  "Cannot reach" is decided
// conservatively: the pyramid of rays through the block GROWN BY ONE PIXEL on every side (the jitter of :995-996 keeps a
// sample inside its pixel, at most on its far edge after rounding) is tested in double precision against the eight corners
// of the root box; a block is dropped only if one side plane of that pyramid has the whole box outside it, or the box is
// behind the camera.  One pixel is 5e-4 of the image width; the float rounding of the reference's ray set-up and slab test
// is 1e-7 relative, so a ray the reference would let into the root box is never culled.  Not applied when the scene has
// spheres (they are tested outside the BVH, :527-548) and not in counting builds (their counters include these samples).
// cost word: bit 31 = the tile has at least one block that is not provably empty; low bits = pixels that see geometry.
// ---------------------------------------------------------------------------------------------------------------
__device__ bool block_footprint_misses_root(const DeviceScene& S, const FrameParams& P, int x0, int ky0) {
    const double o[3] = {P.cam[kCamOrigin + 0], P.cam[kCamOrigin + 1], P.cam[kCamOrigin + 2]};
    const double ulo = (double)(x0 - 1) / (double)(P.width - 1), uhi = (double)(x0 + 9) / (double)(P.width - 1);
    const double vlo = (double)(ky0 - 1) / (double)(P.height - 1), vhi = (double)(ky0 + 9) / (double)(P.height - 1);
    const double us[4] = {ulo, uhi, uhi, ulo}, vs[4] = {vlo, vlo, vhi, vhi};
    double dir[4][3], mid[3] = {0, 0, 0};
    for (int c = 0; c < 4; ++c)
        for (int a = 0; a < 3; ++a) {
            dir[c][a] = ((double)P.cam[kCamLlc + a] + us[c] * (double)P.cam[kCamHorizontal + a] + vs[c] * (double)P.cam[kCamVertical + a]) - o[a];
            mid[a] += dir[c][a];
        }
    double rel[8][3];
    for (int j = 0; j < 8; ++j)
        for (int a = 0; a < 3; ++a) rel[j][a] = (double)((j >> a) & 1 ? S.root_hi[a] : S.root_lo[a]) - o[a];
    bool behind = true;
    for (int j = 0; j < 8; ++j) behind = behind && (mid[0] * rel[j][0] + mid[1] * rel[j][1] + mid[2] * rel[j][2] <= 0.0);
    if (behind) return true;
    for (int c = 0; c < 4; ++c) {
        const double* a = dir[c];
        const double* b = dir[(c + 1) & 3];
        double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
        const double s = n[0] * mid[0] + n[1] * mid[1] + n[2] * mid[2];          // orient the side plane: inside is positive
        if (s == 0.0) continue;                                                   // degenerate pyramid: never cull on it
        if (s < 0.0) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        bool outside = true;
        for (int j = 0; j < 8; ++j) outside = outside && (n[0] * rel[j][0] + n[1] * rel[j][1] + n[2] * rel[j][2] < 0.0);
        if (outside) return true;
    }
    return false;
}

// (batch launches: blockIdx.y is the frame; its camera comes from the batch table and its cost words lie `stride` further on)
__global__ void __launch_bounds__(256) dsrt_tile_cost_kernel(const DeviceScene S, const FrameParams P0, uint32_t* __restrict__ cost, int cull,
                                                             const BatchFrame* __restrict__ batch, uint32_t stride) {
    FrameParams P = P0;
    if (batch) {
        for (int a = 0; a < 12; ++a) P.cam[a] = batch[blockIdx.y].cam[a];
        cost += (size_t)blockIdx.y * stride;
    }
    const uint32_t blocks_per_tile = (uint32_t)((P.tile >> 3) * (P.tile >> 3));
    const uint32_t wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u;
    if (wave_id >= (uint32_t)P.local_tiles * blocks_per_tile) return;
    const uint32_t k = wave_id / blocks_per_tile, sub = wave_id % blocks_per_tile, per_row = (uint32_t)P.tile >> 3;
    const uint32_t g = k * (uint32_t)P.shard_count + (uint32_t)P.shard_rank;
    const uint32_t tx = g % (uint32_t)P.tiles_x, ty = g / (uint32_t)P.tiles_x;
    const int x = (int)(tx * (uint32_t)P.tile + (sub % per_row) * 8u + (lane & 7u));
    const int row = (int)(ty * (uint32_t)P.tile + (sub / per_row) * 8u + (lane >> 3));
    bool hit = false;
    {
        // wave-uniform: this 8x8 block's first column and its lowest kernel row (ky = H - 1 - row; the block's rows are row0..row0+7)
        const int bx0 = (int)(tx * (uint32_t)P.tile + (sub % per_row) * 8u), brow0 = (int)(ty * (uint32_t)P.tile + (sub / per_row) * 8u);
        const bool empty = cull && S.num_spheres == 0 && (S.root_ref == kRefNone || block_footprint_misses_root(S, P, bx0, P.height - 1 - (brow0 + 7)));
        if (empty) return;
        if (lane == 0) atomicOr(&cost[k], 0x80000000u);
    }
    if (x < P.width && row < P.height) {
        const int ky = P.height - 1 - row;
        const float u = ((float)x + 0.5f) / (float)(P.width - 1), v = ((float)ky + 0.5f) / (float)(P.height - 1);
        const F3 ro = ld3(P.cam + kCamOrigin);
        const F3 rd = ((ld3(P.cam + kCamLlc) + (ld3(P.cam + kCamHorizontal) * u)) + (ld3(P.cam + kCamVertical) * v)) - ro;
        const F3 rinv = mk(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
        for (int i = 0; i < S.num_spheres && !hit; ++i) { float t; F3 n; hit = hit_sphere(S.spheres[i], ro, rd, kTMax, t, n); }
        float t_entry;
        if (!hit && S.root_ref != kRefNone && slab(ld3(S.root_lo), ld3(S.root_hi), ro, rinv, kTMax, t_entry)) {
            int stack[64];
            int sp = 0, cur = S.root_ref;
            for (int guard = 0; guard < (1 << 20) && !hit; ++guard) {
                if (cur >= 0) {
                    const float4* rec = S.pairs + (size_t)(cur - kRefBias) * 4;
                    const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
                    float tl, tr;
                    const bool hl = slab(mk(q0.x, q1.x, q2.x), mk(q0.z, q1.z, q2.z), ro, rinv, kTMax, tl);
                    const bool hr = slab(mk(q0.y, q1.y, q2.y), mk(q0.w, q1.w, q2.w), ro, rinv, kTMax, tr);
                    const int rl = __float_as_int(q3.x), rr = __float_as_int(q3.y);
                    if (hl && hr) { if (sp < 64) stack[sp++] = rr; cur = rl; }
                    else if (hl) cur = rl;
                    else if (hr) cur = rr;
                    else { if (sp == 0) break; cur = stack[--sp]; }
                } else {
                    int first = leaf_payload(cur), count = leaf_code(cur) + 1;
                    if (count == 8) { const int2 bl = S.big_leaves[first]; first = bl.x; count = bl.y; }
                    for (int i = 0; i < count && !hit; ++i) {
                        const float* tp = reinterpret_cast<const float*>(S.tri_pairs + (size_t)(first + (i >> 1)) * 5) + (i & 1);
                        const F3 v0 = mk(tp[0], tp[2], tp[4]), e1 = mk(tp[6], tp[8], tp[10]), e2 = mk(tp[12], tp[14], tp[16]);
                        const F3 pvec = cross(rd, e2);
                        const float det = dot(e1, pvec);
                        const float inv_det = 1.0f / det;
                        const F3 tvec = ro - v0;
                        const float uu = dot(tvec, pvec) * inv_det;
                        const F3 qvec = cross(tvec, e1);
                        const float vv = dot(rd, qvec) * inv_det;
                        const float t = dot(e2, qvec) * inv_det;
                        hit = !(fabsf(det) < 1e-8f) && !(uu < 0.0f) && !(uu > 1.0f) && !(vv < 0.0f) && !(uu + vv > 1.0f) && !(t < kTMin) && !(t > kTMax);
                    }
                    if (sp == 0) break;
                    cur = stack[--sp];
                }
            }
        }
    }
    const uint32_t n = (uint32_t)__popcll(wave_ballot(hit));
    if (lane == 0 && n) atomicAdd(&cost[k], n);
}

// One block: counting sort of the shard's live tiles by cost, costliest first (65 bins; order inside a bin does not matter).  bin = 64 - min(64, pixels that see
// geometry * 64 / tile^2); the tiles of bin 64 are the LIGHT tiles, the others -- at least 1/64 of their pixels see geometry -- the HEAVY ones, sched[0] of them.
// (batch launches: one block per frame, the frames' arrays `stride` apart)
__global__ void __launch_bounds__(1024) dsrt_tile_order_kernel(const uint32_t* __restrict__ cost, uint32_t* __restrict__ order, int n, int tile,
                                                               uint32_t* __restrict__ sched, uint32_t items_per_pixel, uint32_t resident_lanes, int spp, uint32_t stride) {
    cost += (size_t)blockIdx.x * stride; order += (size_t)blockIdx.x * stride; sched += (size_t)blockIdx.x * stride;
    __shared__ uint32_t bins[65], cursor[65];
    const uint32_t full = (uint32_t)(tile * tile);
    for (int b = threadIdx.x; b < 65; b += blockDim.x) bins[b] = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += blockDim.x)
        if (cost[t]) atomicAdd(&bins[64u - min(64u, (cost[t] & 0x7FFFFFFFu) * 64u / full)], 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int b = 0; b < 65; ++b) { cursor[b] = acc; acc += bins[b]; }
        const uint32_t n_heavy = acc - bins[64];
        // lanes per wave that start on the heavy queue: all of them once the heavy items outnumber the resident lanes, otherwise
        // just enough to deal the heavy items out over every resident wave (see ST_FETCH in path_machine.h)
        // rng_mode 1 (items_per_pixel > 1): how many slices a heavy pixel is cut into.  8 when the heavy pixels alone fill the chip; with
        // fewer of them (a far frame) up to 64, so that their work spreads over more WAVES -- sample stealing only evens out a wave
        uint32_t slices = items_per_pixel, chunk_len = spp;
        if (items_per_pixel > 1u) {
            const unsigned long long heavy_pixels = (unsigned long long)n_heavy * full;
            while (slices < 64u && slices * 2u <= (uint32_t)spp && heavy_pixels * slices * 2ull <= resident_lanes) slices *= 2u;
            chunk_len = ((uint32_t)spp + slices - 1u) / slices;
            slices = ((uint32_t)spp + chunk_len - 1u) / chunk_len;
        }
        const unsigned long long heavy_items = (unsigned long long)n_heavy * full * slices;
        uint32_t spread = 64;
        if (heavy_items < resident_lanes) spread = (uint32_t)((heavy_items * 64ull + resident_lanes - 1) / resident_lanes);
        sched[0] = n_heavy; sched[1] = acc; sched[2] = spread < 1 ? 1u : spread; sched[3] = slices; sched[4] = chunk_len;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < n; t += blockDim.x)
        if (cost[t]) order[atomicAdd(&cursor[64u - min(64u, (cost[t] & 0x7FFFFFFFu) * 64u / full)], 1u)] = (uint32_t)t;
}

// Refinement of the order by measured cost: a probe launch of the render kernel itself (a few samples per pixel, same state
// machine) has left the number of rays it traced for every tile in `work`; the heavy tiles -- the first sched[0]
// entries of `order` -- are re-sorted by it, most work first, so the pixels with the longest serial sample chains start at
// once instead of wherever their tile's coverage count put them.  Scheduling only.
__global__ void __launch_bounds__(1024) dsrt_tile_reorder_kernel(const uint32_t* __restrict__ work, uint32_t* __restrict__ order, uint32_t* __restrict__ tmp,
                                                                 const uint32_t* __restrict__ sched) {
    __shared__ uint32_t bins[256], cursor[256], wmax;
    const uint32_t n = sched[0];
    // Fewer heavy pixels than resident lanes (a mid-distance frame; one rank's share): every heavy pixel starts in the first instant
    // whatever the order, and the order only decides which waves -- fetching at the same moment, so mostly neighbours on a CU --
    // hold the long chains.  Sorted, the costliest tiles sit side by side; dealt costliest, cheapest, second costliest, ... a long
    // chain's neighbours finish early and leave it the SIMD.  Interleaved medians at 1080p x 1000 (sorted / dealt / coverage order /
    // no probe): frame 75 387 / 361 / 374 / 374 ms, frame 85 400 / 388 / 368 / 373, frame 90 505 / 500 / 512 / 479, one of 8 shares of
    // the near frame 564 / 563 / 625 / 610 (profiles/r02/ab_small_regime_order.jsonl); one setting spreads +-5 % on such frames.
    const bool all_start_at_once = sched[2] < 64u;
    for (int b = threadIdx.x; b < 256; b += blockDim.x) bins[b] = 0;
    if (threadIdx.x == 0) wmax = 1u;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) atomicMax(&wmax, work[order[i]]);
    __syncthreads();
    const uint32_t top = wmax;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        tmp[i] = order[i];
        atomicAdd(&bins[255u - (uint32_t)((unsigned long long)work[order[i]] * 255ull / top)], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t acc = 0; for (int b = 0; b < 256; ++b) { cursor[b] = acc; acc += bins[b]; } }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t t = tmp[i];
        order[atomicAdd(&cursor[255u - (uint32_t)((unsigned long long)work[t] * 255ull / top)], 1u)] = t;
    }
    if (all_start_at_once) {             // costliest, cheapest, second costliest, second cheapest, ...
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) tmp[i] = order[i];
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) order[i] = (i & 1u) ? tmp[n - 1u - (i >> 1)] : tmp[i >> 1];
    }
}

hipError_t launch_tile_reorder(const uint32_t* work, uint32_t* order, uint32_t* tmp, const uint32_t* sched, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_tile_reorder_kernel, dim3(1), dim3(1024), 0, stream, work, order, tmp, sched);
    return hipGetLastError();
}

hipError_t launch_tile_order(const DeviceScene& S, const FrameParams& P, uint32_t* cost, uint32_t* order, uint32_t* sched, uint32_t items_per_pixel,
                             uint32_t resident_lanes, bool cull, hipStream_t stream, const BatchFrame* batch, uint32_t frames, uint32_t stride) {
    const uint32_t waves = (uint32_t)P.local_tiles * (uint32_t)((P.tile >> 3) * (P.tile >> 3));
    for (uint32_t f = 0; f < frames; ++f) {                           // (the cost words only: the arrays carry the sched words behind them)
        hipError_t e = hipMemsetAsync(cost + (size_t)f * stride, 0, (size_t)P.local_tiles * sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(dsrt_tile_cost_kernel, dim3((waves + 3) / 4, frames), dim3(256), 0, stream, S, P, cost, cull ? 1 : 0, batch, stride);
    hipLaunchKernelGGL(dsrt_tile_order_kernel, dim3(frames), dim3(1024), 0, stream, (const uint32_t*)cost, order, P.local_tiles, P.tile, sched, items_per_pixel, resident_lanes, P.spp, stride);
    return hipGetLastError();
}

hipError_t launch_tile_order_arrays(const uint32_t* cost, uint32_t* order, int n, int tile, uint32_t* sched, uint32_t items_per_pixel, uint32_t resident_lanes, int spp,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_tile_order_kernel, dim3(1), dim3(1024), 0, stream, cost, order, n, tile, sched, items_per_pixel, resident_lanes, spp, 0u);
    return hipGetLastError();
}

hipError_t launch_batch_table(BatchFrame* table, const uint32_t* sched, uint32_t sched_stride, uint32_t frames, uint32_t tt, int rng_mode, int spp, int light_chunk_len,
                              uint32_t* total_items, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_batch_table_kernel, dim3(1), dim3(64), 0, stream, table, sched, sched_stride, frames, tt, rng_mode, spp, light_chunk_len, total_items);
    return hipGetLastError();
}

}  // namespace dsrt
