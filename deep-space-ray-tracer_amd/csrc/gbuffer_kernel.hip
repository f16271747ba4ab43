// gbuffer_kernel.hip -- the ground-truth G-buffer pass (include/dsrt.h, dsrt_render_gbuffer): one primary ray per pixel through the pixel centre,
// its first hit as scene_hit(ray, 0.001f, 1e9f) of the reference's ray_color returns it (src/gpu_render.cu:744), the per-pixel channels of that
// hit, and whether the hit sees the Sun (the shadow ray of :800-810).
//
//   * One lane per pixel, one 8x8 pixel tile per wave (a 64-thread workgroup): primary rays of a wave are coherent.
//   * The walk is the reference's, on the REFERENCE tree (DeviceScene.root_ref) even when the certified second tree is resident: near child first
//     by the render kernel's ordering test, far child pushed, LIFO pop, a leaf's triangles in leaf order, every box tested against the shrinking
//     `closest`.  Equal t is accepted (:353), so ties resolve as in the reference.  The per-record arithmetic is the render kernel's own
//     (walk_common.h: walk_reference_tree, visit_pair, moller_trumbore_pair); spheres follow the tree, in order, as in scene_hit :527-548.
//   * What follows the walk -- the hit's record, the spheres, the shadow ray's any-hit tail, the channel stores -- is hit_record.h's, shared with the coverage
//     pass and the ray queries: finish_scene_hit, any_hit_blocked, store_hit.
//   * The traversal stack lives in LDS, [entry][lane] like the render kernel's, sized per launch by the tree's depth (DeviceScene.stack_need,
//     at most 64: dsrt_scene_upload refuses deeper trees): no runtime-indexed private array, hence no scratch.
//   * Second phase of the same launch: the lanes whose hit faces the Sun trace the shadow ray as an any-hit walk.  It stops at the first accepted
//     triangle: until then it performs exactly the closest-hit walk's steps (closest is still 1e9 in both), so "blocked" is scene_hit's boolean.
//   * No sinf / cosf / powf on this path: compiled once, whatever DsrtRenderDesc.math_mode says.
#include "hit_record.h"
#include "launchers.h"

namespace dsrt {

__global__ void __launch_bounds__(64) dsrt_gbuffer_kernel(const GBufferArgs a) {
    extern __shared__ uint2 gb_stack[];                                      // [entry][lane]
    const DeviceScene& S = a.scene;
    const int lane = threadIdx.x;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const int x = tx * 8 + (lane & 7), row = ty * 8 + (lane >> 3);
    const bool live = x < a.width && row < a.height;
    uint2* stk = gb_stack + lane;
    uint32_t status = 0;

    // ---- phase 1: the primary ray, make_camera_ray_jittered :941-968 with jx = jy = 0.5; rows top first (kernel row ky = H-1-row, :984, :1027) ----
    const int ky = a.height - 1 - row;
    const float u = ((float)x + 0.5f) / (float)(a.width - 1), v = ((float)ky + 0.5f) / (float)(a.height - 1);
    const F3 ro = ld3(a.cam + kCamOrigin);
    const F3 rd = ((ld3(a.cam + kCamLlc) + (ld3(a.cam + kCamHorizontal) * u)) + (ld3(a.cam + kCamVertical) * v)) - ro;
    const F3 rinv = mk(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
    float closest = kTMax, hu = 0.0f, hv = 0.0f;
    int slot = -1;
    if (live) walk_reference_tree<false>(S, stk, a.stack_entries, ro, rd, rinv, kTMin, closest, slot, hu, hv, status);

    // ---- finish scene_hit :516-551 (hit_record.h): the triangle's record from (slot, t, u, v), then the spheres ----
    const HitRecord h = finish_scene_hit(S, ro, rd, kTMin, closest, slot, hu, hv, live, status);
    const bool hit = h.hit;

    // ---- the Sun: cos_theta of :800-806 and the shadow ray's start ----
    float cos_t = 0.0f;
    F3 ldir = mk(0, 0, 0);
    if (a.sun_enabled) {
        ldir = normalize(mk(-a.sun_dir[0], -a.sun_dir[1], -a.sun_dir[2]));
        if (hit) cos_t = fmaxf(0.0f, dot(h.n, ldir));
    }
    bool sun_visible = false;

    // ---- phase 2: the shadow rays (only where asked for and facing the Sun), any-hit, then the spheres (:809-816) ----
    const bool need_shadow = a.flags && hit && cos_t > 0.0f;
    if (__builtin_amdgcn_ballot_w64(need_shadow) != 0ull) {
        if (need_shadow) {
            const F3 so = h.p + (h.n * 1e-3f);
            const F3 sinv = mk(1.0f / ldir.x, 1.0f / ldir.y, 1.0f / ldir.z);
            float s_closest = kTMax, su = 0.0f, sv = 0.0f;
            int s_slot = -1;
            walk_reference_tree<true>(S, stk, a.stack_entries, so, ldir, sinv, kTMin, s_closest, s_slot, su, sv, status);
            sun_visible = !any_hit_blocked(S, so, ldir, kTMin, s_closest, s_slot);
        }
    }

    if (live) {
        const HitChannels ch = {a.t, a.range, a.depth, a.position, a.normal, a.uv, a.albedo, a.prim_id, a.material_id, a.sun_cos, a.flags};
        store_hit(S, ch, (size_t)row * (size_t)a.width + (size_t)x, h, rd, a.neg_w, cos_t, sun_visible);
    }
    if (status) atomicOr(a.status, status);
}

hipError_t launch_gbuffer(const GBufferArgs& a, int tiles, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_gbuffer_kernel, dim3((unsigned)tiles), dim3(64), (size_t)a.stack_entries * 64 * sizeof(uint2), stream, a);
    return hipGetLastError();
}

}  // namespace dsrt
