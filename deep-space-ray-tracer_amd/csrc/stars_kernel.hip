// stars_kernel.hip -- the star field (include/dsrt.h, POINT SOURCES): point sources at infinity, projected through the context's camera, occluded by the resident
// scene and deposited into the linear frame, every output bit fixed by the header and reproduced by tests/_stars_model.py.  Three kernels:
//
//   * project    one lane per star: the projection of TEMPORAL ACCUMULATION with the star's direction in place of X_p - C.origin.  The indices of the projected
//                stars are appended to a list -- one ballot per wave and ONE atomic per workgroup of sixteen waves for its slots; a lane's place among its
//                wave's is the count of set ballot bits below it.  A whole-sky catalogue has a few percent of its stars in the field of view: the walk that
//                follows then runs on full waves of projected stars, not on waves with four live lanes.  The list's order depends on which workgroup's atomic
//                came first and does not matter: nothing downstream depends on it (see deposit).  A star that is not projected gets its per-star outputs here.
//   * deposit    one lane per LISTED star: the projection again (the same function, so the same bits; cheaper than a round trip through memory), the any-hit
//                walk of the ray queries (walk_common.h: walk_reference_tree<true>, then hit_record.h: any_hit_blocked) with the stack in dynamic LDS, [entry][lane],
//                sized per launch by DeviceScene.stack_need, then up to twelve 64-bit integer atomicAdds -- four taps, three channels -- into the accumulator,
//                and the per-star outputs.  A deposit is a non-negative integer number of quanta of 2^-24, so a pixel's sum is exact and the same in every order:
//                this is what a float atomicAdd cannot give.  The grid covers `count` lanes (the list's length is known on the device only); workgroups beyond
//                the list leave at once.
//   * resolve    one streaming pass: layer = (float)A * 2^-24 (one rounding, to nearest even), out = in + layer; a word that held a sum is set back to zero, so the
//                accumulator needs no clearing pass per call (a star field touches a few pixels in a thousand).
//
// Vector atomics (global_atomic_add_x2, global_atomic_add) and plain vector stores only.  No private arrays, no scratch.
// There is no reference counterpart (the reference's sky is black).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, no fast-math, as raycast_kernel.hip.
#include "hit_record.h"
#include "launchers.h"
#include "pixel_arith.h"

namespace dsrt {

namespace {

// include/dsrt.h, POINT SOURCES step 1: TEMPORAL ACCUMULATION's projection of D, operation by operation.  C: origin, lower_left_corner, horizontal, vertical, u, v, w.
__device__ __forceinline__ bool project_star(const float* C, int W, int H, float Dx, float Dy, float Dz, float& fx, float& fy) {
    const float ex = C[3] - C[0], ey = C[4] - C[1], ez = C[5] - C[2];
    const float da = dot3(Dx, Dy, Dz, C[12], C[13], C[14]), db = dot3(Dx, Dy, Dz, C[15], C[16], C[17]), dc = dot3(Dx, Dy, Dz, C[18], C[19], C[20]);
    const float eu = dot3(ex, ey, ez, C[12], C[13], C[14]), ev = dot3(ex, ey, ez, C[15], C[16], C[17]), ew = dot3(ex, ey, ez, C[18], C[19], C[20]);
    const float hu = dot3(C[6], C[7], C[8], C[12], C[13], C[14]), vv = dot3(C[9], C[10], C[11], C[15], C[16], C[17]);
    const float k = ew / dc;
    if (!(k > 0.0f)) return false;
    const float s = (da * k - eu) / hu, t = (db * k - ev) / vv;
    const float px = s * (float)(W - 1) - 0.5f, py = (float)(H - 1) - (t * (float)(H - 1) - 0.5f);
    if (!(px > -1.0f && px < (float)W && py > -1.0f && py < (float)H)) return false;
    fx = px; fy = py;
    return true;
}

}  // namespace

// One lane per star, star blockIdx.x * 1024 + thread.  The workgroup's sixteen waves count their projected stars (one ballot each), the counts meet in LDS, and ONE
// atomic per workgroup reserves the slots: with an atomic per wave, the 2^14 waves of a 2^20-star catalogue queue on the one counter for 0.2 ms (measured), which
// was the pass's largest part.
constexpr int kProjectThreads = 1024;
__global__ void __launch_bounds__(kProjectThreads) dsrt_stars_project_kernel(const StarsArgs a) {
    __shared__ uint32_t wave_count[kProjectThreads / 64], wave_base[kProjectThreads / 64];
    const uint32_t i = blockIdx.x * (uint32_t)kProjectThreads + threadIdx.x;            // count <= 2^22: no wrap
    bool projected = false;
    if (i < (uint32_t)a.count) {
        const F3 D = ld3(a.dir + (size_t)i * 3);
        float fx, fy;
        projected = project_star(a.cam, a.width, a.height, D.x, D.y, D.z, fx, fy);
        if (!projected) {
            if (a.xy) { a.xy[(size_t)i * 2] = 0.0f; a.xy[(size_t)i * 2 + 1] = 0.0f; }
            if (a.star_status) a.star_status[i] = 0;
        }
    }
    const unsigned long long ballot = __ballot(projected);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
        for (int w = 0; w < kProjectThreads / 64; ++w) { wave_base[w] = total; total += wave_count[w]; }
        const uint32_t base = total ? atomicAdd(a.list_len, total) : 0u;
        for (int w = 0; w < kProjectThreads / 64; ++w) wave_base[w] += base;
    }
    __syncthreads();
    if (projected) a.list[wave_base[wave] + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull))] = i;      // base + rank < list_len <= count: inside the list
}

// One lane per listed star, list entry blockIdx.x * 64 + lane.  The list's length is known on the device only: the grid covers `count` lanes, and a workgroup
// beyond the list's end leaves at once.  (A capped grid striding over the list was built: the loop keeps the camera and the scene's pointers live across the walk
// and spills 39 scalar registers; this form spills none.)
__global__ void __launch_bounds__(64) dsrt_stars_deposit_kernel(const StarsArgs a) {
    extern __shared__ uint2 st_stack[];                                      // [entry][lane]
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    const uint32_t listed = min(*a.list_len, (uint32_t)a.count);             // (never more than count; the clamp keeps a stray word from leading outside the list)
    uint32_t status = 0;
    if (j < listed) {
        const uint32_t i = a.list[j];
        if (i < (uint32_t)a.count) {
            const F3 rd = ld3(a.dir + (size_t)i * 3);
            const int W = a.width, H = a.height;
            float fx = 0.0f, fy = 0.0f;
            if (project_star(a.cam, W, H, rd.x, rd.y, rd.z, fx, fy)) {       // true for every listed star: the same function on the same words
                bool blocked = false;
                if (a.occlusion) {
                    const F3 ro = mk(a.cam[0], a.cam[1], a.cam[2]);
                    const F3 rinv = mk(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
                    float closest = kTMax, hu = 0.0f, hv = 0.0f;
                    int slot = -1;
                    walk_reference_tree<true>(a.scene, st_stack + threadIdx.x, a.stack_entries, ro, rd, rinv, kTMin, closest, slot, hu, hv, status);
                    blocked = any_hit_blocked(a.scene, ro, rd, kTMin, closest, slot);
                }
                const float flx = floorf(fx), fly = floorf(fy);
                const int x0 = (int)flx, y0 = (int)fly;                      // in [-1, W-1] x [-1, H-1]
                const bool inside = x0 >= 0 && x0 + 1 < W && y0 >= 0 && y0 + 1 < H;
                if (!blocked && a.acc) {
                    const float wx = fx - flx, wy = fy - fly, ox = 1.0f - wx, oy = 1.0f - wy;
                    const float bw[4] = {ox * oy, wx * oy, ox * wy, wx * wy};
                    const F3 fl = ld3(a.flux + (size_t)i * 3);
                    const float f3[3] = {fl.x, fl.y, fl.z};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int qx = x0 + (q & 1), qy = y0 + (q >> 1);
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;       // flux falls off the edge
                        unsigned long long* px = a.acc + ((size_t)qy * (size_t)W + (size_t)qx) * 3;
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const float d = f3[k] * bw[q];
                            const float qf = fminf(fmaxf(d * 16777216.0f, 0.0f), 1099511627776.0f);
                            const unsigned long long n = (unsigned long long)qf;
                            if (n) atomicAdd(px + k, n);
                        }
                    }
                }
                if (a.xy) { a.xy[(size_t)i * 2] = fx; a.xy[(size_t)i * 2 + 1] = fy; }
                if (a.star_status) a.star_status[i] = (uint8_t)(1u | (blocked ? 0u : 2u) | (inside ? 4u : 0u));
            }
        }
    }
    if (status) atomicOr(a.status, status);
}

// One lane per float of the frame.
__global__ void __launch_bounds__(256) dsrt_stars_resolve_kernel(unsigned long long* acc, const float* linear_in, float* layer, float* linear_out, size_t n) {
    const size_t e = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= n) return;
    const unsigned long long A = acc[e];
    if (A) acc[e] = 0;                                                        // the accumulator is handed back all zeros: the next call has nothing to clear
    const float l = (float)A * 0x1p-24f;
    if (layer) layer[e] = l;
    if (linear_out) linear_out[e] = linear_in[e] + l;
}

hipError_t launch_stars(const StarsArgs& a, hipStream_t stream) {
    if (a.count > 0) {
        const unsigned waves = (unsigned)(((size_t)a.count + 63) / 64);
        hipLaunchKernelGGL(dsrt_stars_project_kernel, dim3((unsigned)(((size_t)a.count + kProjectThreads - 1) / kProjectThreads)), dim3(kProjectThreads), 0, stream, a);
        if (hipError_t e = hipGetLastError()) return e;
        hipLaunchKernelGGL(dsrt_stars_deposit_kernel, dim3(waves), dim3(64), (size_t)a.stack_entries * 64 * sizeof(uint2), stream, a);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (a.acc) {
        const size_t n = (size_t)a.width * (size_t)a.height * 3;            // < 3 * 2^31: the grid fits
        hipLaunchKernelGGL(dsrt_stars_resolve_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a.acc, a.linear_in, a.layer, a.linear_out, n);
    }
    return hipGetLastError();
}

}  // namespace dsrt
