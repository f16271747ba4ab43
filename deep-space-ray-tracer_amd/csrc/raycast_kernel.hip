// raycast_kernel.hip -- batched ray queries on the resident scene (include/dsrt.h, dsrt_trace_rays): for each caller-supplied ray i, the reference's
// scene_hit(ray_i, t_min_i, t_max_i) (src/gpu_render.cu:509-551), bit for bit, or its boolean alone.
//
//   * The walk is the G-buffer pass's (walk_common.h: walk_reference_tree), on the REFERENCE tree (DeviceScene.root_ref) even when the certified second
//     tree is resident, with the ray's own t_min in every place the reference uses it: the slab entry, Moller-Trumbore's `t < t_min` and hit_sphere's two
//     root tests.  `closest` starts at the ray's t_max.  Spheres follow the tree, in order; equal t is accepted, so ties resolve by the reference's visit order.
//   * Closest hit: the G-buffer's channels for the ray.  Any hit: the walk stops at the first accepted triangle, then the spheres; until that accept it takes
//     exactly the closest-hit walk's steps (same `closest` = t_max), so "something was accepted" is scene_hit's boolean.
//   * One lane per ray, a 64-thread workgroup, rays in the caller's order (packed float[3]); the traversal stack in dynamic LDS, [entry][lane], sized per launch
//     by DeviceScene.stack_need: no private arrays, no scratch.
//   * A lane-refill form (persistent waves that hand finished lanes new ray indices) was built and measured: +13 % on incoherent rays, -20 % on coherent
//     ones, so it is not kept.
#include "launchers.h"
#include "walk_common.h"

namespace dsrt {

constexpr uint32_t kRayHit = 1u, kRayFront = 2u, kRaySphere = 4u;     // DSRT_GB_HIT, DSRT_GB_FRONT_FACE, DSRT_GB_SPHERE of include/dsrt.h

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
        bool blocked = slot >= 0;
        for (int k = 0; !blocked && k < S.num_spheres; ++k) {
            float t_hit; F3 n_hit;
            blocked = hit_sphere(S.spheres[k], ro, rd, t_min, closest, t_hit, n_hit);
        }
        a.flags[i] = (uint8_t)(blocked ? kRayHit : 0u);                       // the only channel of an any-hit query
        return;
    }
    bool hit = false, front = false, sphere = false;
    F3 hp = mk(0, 0, 0), hn = mk(0, 0, 0);
    int mat_id = -1, tex_id = -1, prim = -1;
    if (slot >= 0) {
        const float4* sh = S.tri_shade + (size_t)slot * 3;
        const float4 a0 = sh[0], a1 = sh[1], a2 = sh[2];
        const float t = closest;
        hp = mk(ro.x + t * rd.x, ro.y + t * rd.y, ro.z + t * rd.z);
        const float wgt = 1.0f - hu - hv;                                    // :359-369
        F3 n = ((mk(a0.x, a0.y, a0.z) * wgt) + (mk(a0.w, a1.x, a1.y) * hu)) + (mk(a1.z, a1.w, a2.x) * hv);
        n = normalize(n);
        front = dot(rd, n) < 0.0f;
        hn = front ? n : (n * -1.0f);
        mat_id = __float_as_int(a2.y);
        tex_id = __float_as_int(a2.z);
        prim = __float_as_int(a2.w);
        hit = true;
    }
    for (int k = 0; k < S.num_spheres; ++k) {
        const GPUSphere sph = S.spheres[k];
        float t_hit; F3 n_hit;
        if (hit_sphere(sph, ro, rd, t_min, closest, t_hit, n_hit)) {
            hit = true; sphere = true;
            closest = t_hit;
            hp = mk(ro.x + t_hit * rd.x, ro.y + t_hit * rd.y, ro.z + t_hit * rd.z);
            front = dot(rd, n_hit) < 0.0f;
            hn = front ? n_hit : (n_hit * -1.0f);
            mat_id = sph.material_id;
            tex_id = -1;
            prim = -2 - k;
            hu = 0.0f; hv = 0.0f;
        }
    }
    if (hit && (unsigned)mat_id >= (unsigned)S.num_materials) { status |= kFlagBadMaterial; hit = false; }
    const float inf = __builtin_inff();
    if (a.t) a.t[i] = hit ? closest : inf;
    if (a.range) a.range[i] = hit ? closest * sqrtf(dot(rd, rd)) : inf;
    if (a.position) { float* o = a.position + (size_t)i * 3; o[0] = hit ? hp.x : 0.0f; o[1] = hit ? hp.y : 0.0f; o[2] = hit ? hp.z : 0.0f; }
    if (a.normal) { float* o = a.normal + (size_t)i * 3; o[0] = hit ? hn.x : 0.0f; o[1] = hit ? hn.y : 0.0f; o[2] = hit ? hn.z : 0.0f; }
    if (a.uv) { float* o = a.uv + (size_t)i * 2; o[0] = hit ? hu : 0.0f; o[1] = hit ? hv : 0.0f; }
    if (a.albedo) {
        F3 alb = mk(0, 0, 0);
        if (hit) {
            const float4 m1 = S.materials[(size_t)mat_id * 3 + 1];
            alb = mk(m1.x, m1.y, m1.z);                                      // :763-774
            if (tex_id >= 0 && S.tri_uv) {
                const float4* uvp = S.tri_uv + (size_t)slot * 2;
                const float4 u0 = uvp[0], u1 = uvp[1];
                const float wgt = 1.0f - hu - hv;
                const float u_tex = wgt * u0.x + hu * u0.z + hv * u1.x;
                const float v_tex = wgt * u0.y + hu * u0.w + hv * u1.y;
                uint32_t n_fetch = 0;
                alb = alb * tex2d(S, tex_id, u_tex, v_tex, n_fetch);
            }
        }
        float* o = a.albedo + (size_t)i * 3; o[0] = alb.x; o[1] = alb.y; o[2] = alb.z;
    }
    if (a.prim_id) a.prim_id[i] = hit ? prim : -1;
    if (a.material_id) a.material_id[i] = hit ? mat_id : -1;
    if (a.flags) a.flags[i] = (uint8_t)(hit ? (kRayHit | (front ? kRayFront : 0u) | (sphere ? kRaySphere : 0u)) : 0u);
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
