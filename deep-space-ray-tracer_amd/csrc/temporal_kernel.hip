// temporal_kernel.hip -- the temporal accumulation stage of include/dsrt.h (TEMPORAL ACCUMULATION): one thread per pixel, between the denoiser's prepare and its
// first a-trous launch (denoise_kernel.hip).  Three kernels, ONE pixel body, temporal_pixel<kMotion, kShaded>, with two switches over `if constexpr`, as
// denoise_prepare<HAS_ALPHA> is written: a change to the stage is made once.
//
// The body:
//   * It reads the records prepare wrote for its own pixel -- cl = {c, L(c)}, vl = {v, L(v)}, nr = {N, range}, xf = {X, F} -- projects X through the previous
//     frame's camera, gathers the four history records around the projected point, blends, and writes cl / vl IN PLACE (each thread touches its own pixel's
//     records only; the history it gathers from is another buffer) with L recomputed for the blended values, as every writer of cl / vl does.
//   * A history record is 64 bytes = four dwordx4 loads at consecutive addresses; neighbouring pixels project to neighbouring points, so a wave's taps fall into
//     neighbouring records.  `next` is written as four dwordx4 stores per lane.  Measured against one a-trous iteration: DESIGN.md section 4.
//   * The occluder guard reads {c, m} and {X} of the up to sixteen records of the 4 x 4 block around the footprint: a surface in front of the pixel's tangent plane
//     there voids the history, unless an accepted tap of weight >= 0.99 proves the point visible (include/dsrt.h).
//   * The camera's eight dot products are per-launch constants, but they are part of the header's fp32 arithmetic: every lane computes them, by the operations
//     written there, rather than have a host compiler's rounding of them enter the contract.
//   * A tap index is formed only from fx in (-1, W) and fy in (-1, H) -- NaN fails that test -- so x0 is in [-1, W-1], and every tap is bounds-checked before its load.
//
// The switches:
//   * kMotion (dsrt_temporal_bodies_kernel; include/dsrt.h, TEMPORAL ACCUMULATION WITH BODIES) puts the motion stage in front: one coalesced prim_id load, the
//     search of at most 15 triangle ranges held in scalar registers, and for a pixel on a moved body six ds_read_b128 of its body's two poses.  (hn, hx) = (N', X')
//     then stand in for the pixel's normal and position wherever it meets the previous frame: the projection, both tap tests, the guard.  A pass of its own would
//     write and re-read 32 bytes per pixel to save about 40 flops.  The optional X' output (prev_position) exists with this switch only.
//   * kShaded (dsrt_temporal_shaded_kernel; include/dsrt.h, TEMPORAL ACCUMULATION THAT FOLLOWS SHADING; always with kMotion) adds the sun state: s_p from the
//     pixel's own flags byte into word 15 of `next` (0.0f without the switch); the state of a history record is the .w of the X row that the taps and the occluder
//     guard load anyway, so the tap test and edge_prev cost no history traffic; edge_cur is nine byte loads of `flags`, whose lines neighbouring lanes share; the
//     optional status is one byte store per lane.  Here prim_id may be null (a static scene): every pixel is body 0 and the motion stage is skipped.
//   * An argument a kernel does not have (mo, sh, pose_lds) is passed as nullptr and touched only under its switch.
//
// There is no reference counterpart (the reference reconstructs outside its renderer).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off, no fast-math, as denoise_kernel.hip.
#include <cfloat>

#include "launchers.h"
#include "pixel_arith.h"

namespace dsrt {

namespace {
template <bool kMotion, bool kShaded>
__device__ __forceinline__ void temporal_pixel(const TemporalArgs& a, const BodyMotionArgs* mo, const ShadingArgs* sh, const float4* pose_lds) {
    static_assert(kMotion || !kShaded, "the sun state comes with the motion stage");
    const int x = (int)blockIdx.x * 16 + (int)(threadIdx.x & 15u), y = (int)blockIdx.y * 16 + (int)(threadIdx.x >> 4);
    const int W = a.width, H = a.height;
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    const float4 cp = a.cl[p], vp = a.vl[p], np = a.nr[p], xp = a.xf[p];
    float hnx = np.x, hny = np.y, hnz = np.z, hxx = xp.x, hxy = xp.y, hxz = xp.z;
    if constexpr (kMotion) {
        // the pixel's body: at most 15 wave-uniform ranges, from the kernarg (scalar registers); they do not overlap, so the order of the search does not matter
        // (first <= prim < first + count, whatever the sum: with prim >= first >= 0 the difference is below 2^31 and the unsigned test is exact; without that
        // comparison a negative prim_id would wrap into a range that reaches beyond 2^31)
        if (!kShaded || mo->prim_id) {                                       // (the bodies kernel's API requires prim_id; else uniform over the launch)
            const int32_t prim = mo->prim_id[p];
            int body = 0;
#pragma unroll
            for (int b = 1; b < kMaxBodies; ++b) body = ((prim >= mo->first[b]) & ((uint32_t)prim - (uint32_t)mo->first[b] < (uint32_t)mo->count[b])) ? b : body;
            if (mo->moved >> body & 1u) {                                    // (bit 0 is never set)
                const float4* t = pose_lds + body * 6;                       // cur rows 0..2, prev rows 0..2: {r0 r1 r2 t}
                const float4 c0 = t[0], c1 = t[1], c2 = t[2], q0 = t[3], q1 = t[4], q2 = t[5];
                const float dx = xp.x - c0.w, dy = xp.y - c1.w, dz = xp.z - c2.w;
                const float rx = (c0.x * dx + c1.x * dy) + c2.x * dz, ry = (c0.y * dx + c1.y * dy) + c2.y * dz, rz = (c0.z * dx + c1.z * dy) + c2.z * dz;
                const float mx = (c0.x * np.x + c1.x * np.y) + c2.x * np.z, my = (c0.y * np.x + c1.y * np.y) + c2.y * np.z, mz = (c0.z * np.x + c1.z * np.y) + c2.z * np.z;
                hxx = ((q0.x * rx + q0.y * ry) + q0.z * rz) + q0.w; hxy = ((q1.x * rx + q1.y * ry) + q1.z * rz) + q1.w; hxz = ((q2.x * rx + q2.y * ry) + q2.z * rz) + q2.w;
                hnx = (q0.x * mx + q0.y * my) + q0.z * mz; hny = (q1.x * mx + q1.y * my) + q1.z * mz; hnz = (q2.x * mx + q2.y * my) + q2.z * mz;
            }
        }
    }
    const bool filterable = xp.w != 0.0f;
    const float nf = (float)(a.counts ? a.counts[p] : (uint32_t)a.samples_done);
    const float qnan = __uint_as_float(0x7FC00000u);
    float sp = 0.0f;                                                         // the sun state: 0 unknown (a miss, or no shading), 1 in shadow, 2 lit
    bool edge_cur = false;
    if constexpr (kShaded) {
        const uint32_t fp = sh->flags[p];
        sp = np.w <= FLT_MAX ? ((fp & 8u) ? 2.0f : 1.0f) : 0.0f;
        // the current frame's edge: a hit among the 3 x 3 neighbours whose sun bit is not this pixel's (bounds-checked byte loads of the caller's flags; formed
        // here, for every pixel, so that nothing of it but the one bit lives through the taps)
        for (int ny = y - 1; ny <= y + 1; ++ny) {
            if (ny < 0 || ny >= H) continue;
            for (int nx = x - 1; nx <= x + 1; ++nx) {
                if (nx < 0 || nx >= W) continue;
                const uint32_t fr = sh->flags[(size_t)ny * (size_t)W + (size_t)nx];
                edge_cur |= (fr & 1u) && ((fr ^ fp) & 8u);
            }
        }
    }

    // ---- the projection into the previous frame ----
    float fx = qnan, fy = qnan;
    bool projected = false;
    if (a.prev && np.w <= FLT_MAX) {
        const float* C = a.cam;                                              // origin, lower_left_corner, horizontal, vertical, u, v, w
        const float Dx = hxx - C[0], Dy = hxy - C[1], Dz = hxz - C[2];
        const float ex = C[3] - C[0], ey = C[4] - C[1], ez = C[5] - C[2];
        const float da = dot3(Dx, Dy, Dz, C[12], C[13], C[14]), db = dot3(Dx, Dy, Dz, C[15], C[16], C[17]), dc = dot3(Dx, Dy, Dz, C[18], C[19], C[20]);
        const float eu = dot3(ex, ey, ez, C[12], C[13], C[14]), ev = dot3(ex, ey, ez, C[15], C[16], C[17]), ew = dot3(ex, ey, ez, C[18], C[19], C[20]);
        const float hu = dot3(C[6], C[7], C[8], C[12], C[13], C[14]), vv = dot3(C[9], C[10], C[11], C[15], C[16], C[17]);
        const float k = ew / dc;
        if (k > 0.0f) {
            const float s = (da * k - eu) / hu, t = (db * k - ev) / vv;
            const float px = s * (float)(W - 1) - 0.5f, py = (float)(H - 1) - (t * (float)(H - 1) - 0.5f);
            if (px > -1.0f && px < (float)W && py > -1.0f && py < (float)H) { fx = px; fy = py; projected = true; }
        }
    }

    // ---- the four taps ----
    float c0 = cp.x, c1 = cp.y, c2 = cp.z, v0 = vp.x, v1 = vp.y, v2 = vp.z;
    float m = filterable ? nf : 0.0f;
    uint32_t status = projected ? 1u : 0u;
    if (projected && filterable) {
        const float flx = floorf(fx), fly = floorf(fy);
        const int x0 = (int)flx, y0 = (int)fly;                              // in [-1, W-1] x [-1, H-1]
        const float wx = fx - flx, wy = fy - fly, ox = 1.0f - wx, oy = 1.0f - wy;
        const float bw[4] = {ox * oy, wx * oy, ox * wy, wx * wy};
        const float tol = a.plane_tol * np.w;
        // the occluder guard: a record of the 4 x 4 block around the footprint that holds a surface in FRONT of this pixel's tangent plane voids the history;
        // with the sun state, over the same records, the previous frame's edge: a usable record whose sun state is not this pixel's
        bool guarded = false, edge_prev = false;
        for (int gy = y0 - 1; gy <= y0 + 2; ++gy) {
            if (gy < 0 || gy >= H) continue;
            for (int gx = x0 - 1; gx <= x0 + 2; ++gx) {
                if (gx < 0 || gx >= W) continue;
                const float4* rec = a.prev + ((size_t)gy * (size_t)W + (size_t)gx) * 4;
                const float4 cq = rec[0], xq = rec[3];
                guarded |= cq.w > 0.0f && dot3(hnx, hny, hnz, xq.x - hxx, xq.y - hxy, xq.z - hxz) > tol;
                if constexpr (kShaded) edge_prev |= cq.w > 0.0f && !(xq.w == 0.0f || xq.w == sp);
            }
        }
        float sw = 0.0f, sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f, sv0 = 0.0f, sv1 = 0.0f, sv2 = 0.0f, sm = 0.0f, swg = 0.0f;
        bool seen = false, seen_g = false;                                   // an accepted tap whose centre ray all but coincides with the ray to X: proof of visibility
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float4* rec = a.prev + ((size_t)qy * (size_t)W + (size_t)qx) * 4;
            const float4 cq = rec[0], vq = rec[1], nq = rec[2], xq = rec[3];
            if (!(cq.w > 0.0f)) continue;
            if (!(dot3(hnx, hny, hnz, nq.x, nq.y, nq.z) >= a.normal_cos_min)) continue;
            if (!(fabsf(dot3(hnx, hny, hnz, xq.x - hxx, xq.y - hxy, xq.z - hxz)) <= tol)) continue;
            const float b = bw[k];
            if constexpr (kShaded) {
                seen_g |= b >= 0.99f;                                        // what the stage without the sun state would have accumulated
                swg += b;
                if (!(xq.w == 0.0f || xq.w == sp)) continue;                 // a record of the other sun state (NaN: of no state)
            }
            seen |= b >= 0.99f;
            sw += b;
            sc0 += b * cq.x; sc1 += b * cq.y; sc2 += b * cq.z;
            sv0 += b * vq.x; sv1 += b * vq.y; sv2 += b * vq.z;
            sm += b * cq.w;
        }
        bool found = sw >= a.min_support && (seen || !guarded);
        if constexpr (kShaded) {
            const bool found_geometry = swg >= a.min_support && (seen_g || !guarded);
            found = found && !(sh->edge_guard && (edge_prev || edge_cur));
            status |= (found ? 2u : 0u) | (found_geometry ? 4u : 0u) | (edge_prev ? 8u : 0u) | (edge_cur ? 16u : 0u);
        }
        if (found) {
            const float mh = sm / sw;
            const float alpha = fmaxf(nf / (nf + mh), a.alpha_min), beta = 1.0f - alpha;
            const float b2 = beta * beta, a2 = alpha * alpha;
            c0 = beta * (sc0 / sw) + alpha * cp.x; c1 = beta * (sc1 / sw) + alpha * cp.y; c2 = beta * (sc2 / sw) + alpha * cp.z;
            v0 = b2 * (sv0 / sw) + a2 * vp.x; v1 = b2 * (sv1 / sw) + a2 * vp.y; v2 = b2 * (sv2 / sw) + a2 * vp.z;
            m = nf / alpha;
            a.cl[p] = make_float4(c0, c1, c2, lum(c0, c1, c2));
            a.vl[p] = make_float4(v0, v1, v2, lum(v0, v1, v2));
        }
    }

    float4* out = a.next + p * 4;
    out[0] = make_float4(c0, c1, c2, m);
    out[1] = make_float4(v0, v1, v2, 0.0f);
    out[2] = make_float4(np.x, np.y, np.z, 0.0f);
    out[3] = make_float4(xp.x, xp.y, xp.z, sp);
    if (a.prev_xy) { a.prev_xy[p * 2] = fx; a.prev_xy[p * 2 + 1] = fy; }      // (the caller's buffer is 4-byte aligned: two stores)
    if (a.weight) a.weight[p] = m;
    if constexpr (kShaded) if (sh->status) sh->status[p] = (uint8_t)status;
    if constexpr (kMotion) {
        if (mo->prev_position) {                                             // (with the sun state: given with prim_id only)
            const bool hit = np.w <= FLT_MAX;
            float* o = mo->prev_position + p * 3;
            o[0] = hit ? hxx : 0.0f; o[1] = hit ? hxy : 0.0f; o[2] = hit ? hxz : 0.0f;
        }
    }
}

// The pose table -- 16 bodies x 24 floats, 1.5 KB -- comes in the kernarg and is staged in LDS once per workgroup, 96 lanes one float4 each (a coalesced load of
// consecutive kernarg addresses); a pixel on a moved body then reads its body's six float4 with ds_read_b128: lanes of one body read the same address (a
// broadcast), and the index costs neither scratch nor a lane-by-lane walk of the kernarg.  Nothing is staged when no body moved (`moved` is 0 without a motion).
// Every thread of the workgroup calls this: the threads outside the image leave after the barrier.
__device__ __forceinline__ void stage_poses(const BodyMotionArgs& mo, float4* pose_lds) {
    if (mo.moved) {                                                          // (uniform over the launch)
        if (threadIdx.x < kMaxBodies * 6) pose_lds[threadIdx.x] = mo.poses[threadIdx.x];
        __syncthreads();
    }
}
}  // namespace

__global__ __launch_bounds__(256) void dsrt_temporal_kernel(const TemporalArgs a) { temporal_pixel<false, false>(a, nullptr, nullptr, nullptr); }

__global__ __launch_bounds__(256) void dsrt_temporal_bodies_kernel(const TemporalArgs a, const BodyMotionArgs mo) {
    __shared__ float4 pose_lds[kMaxBodies * 6];
    stage_poses(mo, pose_lds);
    temporal_pixel<true, false>(a, &mo, nullptr, pose_lds);
}

__global__ __launch_bounds__(256) void dsrt_temporal_shaded_kernel(const TemporalArgs a, const BodyMotionArgs mo, const ShadingArgs sh) {
    __shared__ float4 pose_lds[kMaxBodies * 6];
    stage_poses(mo, pose_lds);
    temporal_pixel<true, true>(a, &mo, &sh, pose_lds);
}

// Null mo and null sh: the static kernel; sh: the shaded one, whose mo is then required (all zero for a static scene).
hipError_t launch_temporal(const TemporalArgs& a, const BodyMotionArgs* mo, const ShadingArgs* sh, hipStream_t stream) {
    const dim3 grid((unsigned)((a.width + 15) / 16), (unsigned)((a.height + 15) / 16));
    if (sh) hipLaunchKernelGGL(dsrt_temporal_shaded_kernel, grid, dim3(256), 0, stream, a, *mo, *sh);
    else if (mo) hipLaunchKernelGGL(dsrt_temporal_bodies_kernel, grid, dim3(256), 0, stream, a, *mo);
    else hipLaunchKernelGGL(dsrt_temporal_kernel, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace dsrt
