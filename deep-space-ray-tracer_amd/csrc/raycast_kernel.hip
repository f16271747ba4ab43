// raycast_kernel.hip -- batched ray queries on the resident scene (include/dsrt.h, dsrt_trace_rays): for each caller-supplied ray i, the reference's
// scene_hit(ray_i, t_min_i, t_max_i) (src/gpu_render.cu:509-551), bit for bit, or its boolean alone.
//
//   * The walk is the G-buffer pass's (walk_common.h: walk_reference_tree), on the REFERENCE tree (DeviceScene.root_ref) even when the certified second
//     tree is resident, with the ray's own t_min in every place the reference uses it: the slab entry, Moller-Trumbore's `t < t_min` and hit_sphere's two
//     root tests.  `closest` starts at the ray's t_max.  Spheres follow the tree, in order; equal t is accepted, so ties resolve by the reference's visit order.
//   * Closest hit: the G-buffer's channels for the ray, by the G-buffer pass's own code (hit_record.h: finish_scene_hit, store_hit).  Any hit: the walk stops at the first accepted triangle, then the spheres; until that accept it takes
//     exactly the closest-hit walk's steps (same `closest` = t_max), so "something was accepted" is scene_hit's boolean.
//   * One lane per ray, a 64-thread workgroup, rays in the caller's order (packed float[3]); the traversal stack in dynamic LDS, [entry][lane], sized per launch
//     by DeviceScene.stack_need: no private arrays, no scratch.
//   * A lane-refill form (persistent waves that hand finished lanes new ray indices) was built and measured: +13 % on incoherent rays, -20 % on coherent
//     ones, so it is not kept.
#include "hit_record.h"
#include "launchers.h"

namespace dsrt {

__device__ __forceinline__ void load_ray(const RaycastArgs& a, uint32_t i, F3& ro, F3& rd, float& t_min, float& t_max) {
    ro = ld3(a.origins + (size_t)i * 3);
    rd = ld3(a.dirs + (size_t)i * 3);
    t_min = a.t_min ? a.t_min[i] : kTMin;
    t_max = a.t_max ? a.t_max[i] : kTMax;
}

// After the walk: the spheres (scene_hit :527-548), then the ray's channels, defined as in the G-buffer pass.
template <bool ANYHIT>
__device__ __forceinline__ void finish_ray(const RaycastArgs& a, uint32_t i, F3 ro, F3 rd, float t_min, float closest, int slot, float hu, float hv, uint32_t& status) {
    const DeviceScene& S = a.scene;
    if (ANYHIT) {
        a.flags[i] = (uint8_t)(any_hit_blocked(S, ro, rd, t_min, closest, slot) ? kGbHit : 0u);     // the only channel of an any-hit query
        return;
    }
    const HitRecord h = finish_scene_hit(S, ro, rd, t_min, closest, slot, hu, hv, true, status);
    const HitChannels ch = {a.t, a.range, nullptr, a.position, a.normal, a.uv, a.albedo, a.prim_id, a.material_id, nullptr, a.flags};
    store_hit(S, ch, (size_t)i, h, rd, nullptr, 0.0f, false);
}

// One lane per ray, ray blockIdx.x * 64 + lane.
template <bool ANYHIT>
__global__ void __launch_bounds__(64) dsrt_raycast_kernel(const RaycastArgs a) {
    extern __shared__ uint2 rc_stack[];                                      // [entry][lane]
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;                       // count < 2^31: no wrap
    uint32_t status = 0;
    if (i < (uint32_t)a.count) {
        F3 ro, rd;
        float t_min, closest, hu = 0.0f, hv = 0.0f;
        int slot = -1;
        load_ray(a, i, ro, rd, t_min, closest);
        const F3 rinv = mk(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
        walk_reference_tree<ANYHIT>(a.scene, rc_stack + threadIdx.x, a.stack_entries, ro, rd, rinv, t_min, closest, slot, hu, hv, status);
        finish_ray<ANYHIT>(a, i, ro, rd, t_min, closest, slot, hu, hv, status);
    }
    if (status) atomicOr(a.status, status);
}

hipError_t launch_raycast(const RaycastArgs& a, bool any_hit, int blocks, hipStream_t stream) {
    const size_t lds = (size_t)a.stack_entries * 64 * sizeof(uint2);
    if (any_hit) hipLaunchKernelGGL(dsrt_raycast_kernel<true>, dim3((unsigned)blocks), dim3(64), lds, stream, a);
    else hipLaunchKernelGGL(dsrt_raycast_kernel<false>, dim3((unsigned)blocks), dim3(64), lds, stream, a);
    return hipGetLastError();
}

}  // namespace dsrt
