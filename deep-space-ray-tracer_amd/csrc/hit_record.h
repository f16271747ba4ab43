// hit_record.h -- what follows walk_reference_tree (walk_common.h) in the G-buffer pass, the coverage pass and the ray queries, once: the rest of the reference's
// scene_hit (src/gpu_render.cu:516-551) as a finished hit, the any-hit form of the same, and the channels of a hit (include/dsrt.h, DsrtGBuffer) stored at one element.
// This is the code tests/test_gpu_gbuffer.py, test_gpu_coverage.py and test_gpu_trace_rays.py hold to the oracle bit for bit: the operations stand in the
// reference's order and parenthesisation (-ffp-contract=off), and a change here changes all three kernels alike.  The render kernel assembles its record inside
// the path state machine (path_machine.h) and does not use this.
#pragma once

#include "walk_common.h"

namespace dsrt {

constexpr uint32_t kGbHit = 1u, kGbFront = 2u, kGbSphere = 4u, kGbSunVisible = 8u;      // DSRT_GB_* of include/dsrt.h

// A finished scene_hit.  Without a hit: hit false, the rest as the walk and the defaults left it (store_hit writes the miss values).
struct HitRecord {
    bool hit, front, sphere;
    F3 p, n;                   // the point; the normal, turned against the ray
    float t, u, v;
    int slot, mat_id, tex_id, prim;
};

// scene_hit :516-551 after the walk returned (closest, slot, hu, hv): the triangle's record, then the spheres in order (:527-548; `live` gates them, for lanes
// without a ray), then the material check.  `t_min` is the query's lower bound (kTMin for every ray of the G-buffer and coverage passes).
__device__ __forceinline__ HitRecord finish_scene_hit(const DeviceScene& S, F3 ro, F3 rd, float t_min, float closest, int slot, float hu, float hv, bool live, uint32_t& status) {
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
        if (hit_sphere(sph, ro, rd, t_min, closest, t_hit, n_hit)) {
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
    return HitRecord{hit, front, sphere, hp, hn, closest, hu, hv, slot, mat_id, tex_id, prim};
}

// scene_hit's boolean after an any-hit walk: blocked by the walk's triangle, else by the first sphere that blocks (:527-548, :809-816).
__device__ __forceinline__ bool any_hit_blocked(const DeviceScene& S, F3 ro, F3 rd, float t_min, float closest, int slot) {
    bool blocked = slot >= 0;
    for (int i = 0; !blocked && i < S.num_spheres; ++i) {
        float t_hit; F3 n_hit;
        blocked = hit_sphere(S.spheres[i], ro, rd, t_min, closest, t_hit, n_hit);
    }
    return blocked;
}

// The eleven channels of DsrtGBuffer (DsrtRayHits has nine of them: depth and sun_cos stay null), NULL = not written.
struct HitChannels {
    float* t; float* range; float* depth; float* position; float* normal; float* uv; float* albedo;
    int* prim_id; int* material_id; float* sun_cos; uint8_t* flags;
};

// The channels of `h`, the hit of a ray of direction `rd`, at element `p`; a miss writes the miss values of include/dsrt.h.  `neg_w` (the optical axis) is read
// for `depth` only; `cos_t` and `sun_visible` are the caller's Sun terms (0 and false where there are none).
__device__ __forceinline__ void store_hit(const DeviceScene& S, const HitChannels& c, size_t p, const HitRecord& h, F3 rd, const float* neg_w, float cos_t, bool sun_visible) {
    const bool hit = h.hit;
    const float inf = __builtin_inff();
    if (c.t) c.t[p] = hit ? h.t : inf;
    if (c.range) c.range[p] = hit ? h.t * sqrtf(dot(rd, rd)) : inf;
    if (c.depth) c.depth[p] = hit ? h.t * dot(rd, ld3(neg_w)) : inf;
    if (c.position) { float* o = c.position + p * 3; o[0] = hit ? h.p.x : 0.0f; o[1] = hit ? h.p.y : 0.0f; o[2] = hit ? h.p.z : 0.0f; }
    if (c.normal) { float* o = c.normal + p * 3; o[0] = hit ? h.n.x : 0.0f; o[1] = hit ? h.n.y : 0.0f; o[2] = hit ? h.n.z : 0.0f; }
    if (c.uv) { float* o = c.uv + p * 2; o[0] = hit ? h.u : 0.0f; o[1] = hit ? h.v : 0.0f; }
    if (c.albedo) {
        F3 alb = mk(0, 0, 0);
        if (hit) {
            const float4 m1 = S.materials[(size_t)h.mat_id * 3 + 1];
            alb = mk(m1.x, m1.y, m1.z);                                      // :763-774
            if (h.tex_id >= 0 && S.tri_uv) {
                const float4* uvp = S.tri_uv + (size_t)h.slot * 2;
                const float4 u0 = uvp[0], u1 = uvp[1];
                const float wgt = 1.0f - h.u - h.v;
                const float u_tex = wgt * u0.x + h.u * u0.z + h.v * u1.x;
                const float v_tex = wgt * u0.y + h.u * u0.w + h.v * u1.y;
                uint32_t n_fetch = 0;
                alb = alb * tex2d(S, h.tex_id, u_tex, v_tex, n_fetch);
            }
        }
        float* o = c.albedo + p * 3; o[0] = alb.x; o[1] = alb.y; o[2] = alb.z;
    }
    if (c.prim_id) c.prim_id[p] = hit ? h.prim : -1;
    if (c.material_id) c.material_id[p] = hit ? h.mat_id : -1;
    if (c.sun_cos) c.sun_cos[p] = cos_t;
    if (c.flags) c.flags[p] = (uint8_t)(hit ? (kGbHit | (h.front ? kGbFront : 0u) | (h.sphere ? kGbSphere : 0u) | (sun_visible ? kGbSunVisible : 0u)) : 0u);
}

}  // namespace dsrt
