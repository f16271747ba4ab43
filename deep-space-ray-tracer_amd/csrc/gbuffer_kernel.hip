// gbuffer_kernel.hip -- the ground-truth G-buffer pass (include/dsrt.h, dsrt_render_gbuffer): one primary ray per pixel through the pixel centre,
// its first hit as scene_hit(ray, 0.001f, 1e9f) of the reference's ray_color returns it (src/gpu_render.cu:744), the per-pixel channels of that
// hit, and whether the hit sees the Sun (the shadow ray of :800-810).
//
//   * One lane per pixel, one 8x8 pixel tile per wave (a 64-thread workgroup): primary rays of a wave are coherent.
//   * The walk is the reference's, on the REFERENCE tree (DeviceScene.root_ref) even when the certified second tree is resident: near child first
//     by the render kernel's ordering test, far child pushed, LIFO pop, a leaf's triangles in leaf order, every box tested against the shrinking
//     `closest`.  Equal t is accepted (:353), so ties resolve as in the reference.  The per-record arithmetic is the render kernel's own
//     (walk_common.h: walk_reference_tree, visit_pair, moller_trumbore_pair); spheres follow the tree, in order, as in scene_hit :527-548.
//   * The traversal stack lives in LDS, [entry][lane] like the render kernel's, sized per launch by the tree's depth (DeviceScene.stack_need,
//     at most 64: dsrt_scene_upload refuses deeper trees): no runtime-indexed private array, hence no scratch.
//   * Second phase of the same launch: the lanes whose hit faces the Sun trace the shadow ray as an any-hit walk.  It stops at the first accepted
//     triangle: until then it performs exactly the closest-hit walk's steps (closest is still 1e9 in both), so "blocked" is scene_hit's boolean.
//   * No sinf / cosf / powf on this path: compiled once, whatever DsrtRenderDesc.math_mode says.
#include "launchers.h"
#include "walk_common.h"

namespace dsrt {

constexpr uint32_t kGbHit = 1u, kGbFront = 2u, kGbSphere = 4u, kGbSunVisible = 8u;      // DSRT_GB_* of include/dsrt.h

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

    // ---- finish scene_hit :516-551: the triangle's record from (slot, t, u, v), then the spheres ----
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
    for (int i = 0; live && i < S.num_spheres; ++i) {
        const GPUSphere sph = S.spheres[i];
        float t_hit; F3 n_hit;
        if (hit_sphere(sph, ro, rd, closest, t_hit, n_hit)) {
            hit = true; sphere = true;
            closest = t_hit;
            hp = mk(ro.x + t_hit * rd.x, ro.y + t_hit * rd.y, ro.z + t_hit * rd.z);
            front = dot(rd, n_hit) < 0.0f;
            hn = front ? n_hit : (n_hit * -1.0f);
            mat_id = sph.material_id;
            tex_id = -1;
            prim = -2 - i;
            hu = 0.0f; hv = 0.0f;
        }
    }
    if (hit && (unsigned)mat_id >= (unsigned)S.num_materials) { status |= kFlagBadMaterial; hit = false; }

    // ---- the Sun: cos_theta of :800-806 and the shadow ray's start ----
    float cos_t = 0.0f;
    F3 ldir = mk(0, 0, 0);
    if (a.sun_enabled) {
        ldir = normalize(mk(-a.sun_dir[0], -a.sun_dir[1], -a.sun_dir[2]));
        if (hit) cos_t = fmaxf(0.0f, dot(hn, ldir));
    }
    bool sun_visible = false;

    // ---- phase 2: the shadow rays (only where asked for and facing the Sun), any-hit, then the spheres (:809-816) ----
    const bool need_shadow = a.flags && hit && cos_t > 0.0f;
    if (__builtin_amdgcn_ballot_w64(need_shadow) != 0ull) {
        if (need_shadow) {
            const F3 so = hp + (hn * 1e-3f);
            const F3 sinv = mk(1.0f / ldir.x, 1.0f / ldir.y, 1.0f / ldir.z);
            float s_closest = kTMax, su = 0.0f, sv = 0.0f;
            int s_slot = -1;
            walk_reference_tree<true>(S, stk, a.stack_entries, so, ldir, sinv, kTMin, s_closest, s_slot, su, sv, status);
            bool blocked = s_slot >= 0;
            for (int i = 0; !blocked && i < S.num_spheres; ++i) {
                float t_hit; F3 n_hit;
                blocked = hit_sphere(S.spheres[i], so, ldir, s_closest, t_hit, n_hit);
            }
            sun_visible = !blocked;
        }
    }

    if (live) {
        const size_t p = (size_t)row * (size_t)a.width + (size_t)x;
        const float inf = __builtin_inff();
        if (a.t) a.t[p] = hit ? closest : inf;
        if (a.range) a.range[p] = hit ? closest * sqrtf(dot(rd, rd)) : inf;
        if (a.depth) a.depth[p] = hit ? closest * dot(rd, ld3(a.neg_w)) : inf;
        if (a.position) { float* o = a.position + p * 3; o[0] = hit ? hp.x : 0.0f; o[1] = hit ? hp.y : 0.0f; o[2] = hit ? hp.z : 0.0f; }
        if (a.normal) { float* o = a.normal + p * 3; o[0] = hit ? hn.x : 0.0f; o[1] = hit ? hn.y : 0.0f; o[2] = hit ? hn.z : 0.0f; }
        if (a.uv) { float* o = a.uv + p * 2; o[0] = hit ? hu : 0.0f; o[1] = hit ? hv : 0.0f; }
        if (a.albedo) {
            F3 alb = mk(0, 0, 0);
            if (hit) {
                const float4 m1 = S.materials[(size_t)mat_id * 3 + 1];
                alb = mk(m1.x, m1.y, m1.z);                                  // :763-774
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
            float* o = a.albedo + p * 3; o[0] = alb.x; o[1] = alb.y; o[2] = alb.z;
        }
        if (a.prim_id) a.prim_id[p] = hit ? prim : -1;
        if (a.material_id) a.material_id[p] = hit ? mat_id : -1;
        if (a.sun_cos) a.sun_cos[p] = cos_t;
        if (a.flags) a.flags[p] = (uint8_t)(hit ? (kGbHit | (front ? kGbFront : 0u) | (sphere ? kGbSphere : 0u) | (sun_visible ? kGbSunVisible : 0u)) : 0u);
    }
    if (status) atomicOr(a.status, status);
}

hipError_t launch_gbuffer(const GBufferArgs& a, int tiles, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_gbuffer_kernel, dim3((unsigned)tiles), dim3(64), (size_t)a.stack_entries * 64 * sizeof(uint2), stream, a);
    return hipGetLastError();
}

}  // namespace dsrt
