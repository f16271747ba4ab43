// walk_common.h -- the pinned per-record arithmetic of the BVH walk for the kernels other than the render kernel's own loop: one leaf's pair record
// of triangles (moller_trumbore_pair, which render_kernel.hip uses as well) and one internal node's pair record (visit_pair: the node visit of
// render_body, statement for statement -- render_body keeps its copy inline, because a call there, although inlined, changed the render kernel's
// register allocation; tests/test_gpu_gbuffer.py holds the G-buffer pass that uses this one to the oracle bit for bit), and the whole walk on the reference
// tree that the G-buffer pass and the ray queries (raycast_kernel.hip) share.
#pragma once

#include "device_math.h"

namespace dsrt {

// Moller-Trumbore :336-353 on one pair record (two triangles, packed fp32), evaluated in full; the reference's early returns become one
// predicate per triangle.  Each `if (x) return false` is kept as `!(x)` so that NaNs fall the same way.  The test against `closest`
// (:353) is NOT part of this: it is applied, in order, by the caller (render_kernel.hip: apply_pair).
// `t_min` is the query's lower bound (0.001f for every ray of the renderer and the G-buffer: the form without it, below).
__device__ __forceinline__ void moller_trumbore_pair(const float4* __restrict__ tp, F3 ro, F3 rd, float t_min, v2f& t, v2f& u, v2f& v, bool& ok_a, bool& ok_b) {
    const float4 f0 = tp[0], f1 = tp[1], f2 = tp[2], f3 = tp[3];
    const float2 f4 = *reinterpret_cast<const float2*>(tp + 4);
    const v2f v0x = {f0.x, f0.y}, v0y = {f0.z, f0.w}, v0z = {f1.x, f1.y};
    const v2f e1x = {f1.z, f1.w}, e1y = {f2.x, f2.y}, e1z = {f2.z, f2.w};
    const v2f e2x = {f3.x, f3.y}, e2y = {f3.z, f3.w}, e2z = {f4.x, f4.y};
    const v2f pvx = rd.y * e2z - rd.z * e2y, pvy = rd.z * e2x - rd.x * e2z, pvz = rd.x * e2y - rd.y * e2x;   // cross(rd, e2)
    const v2f det = (e1x * pvx + e1y * pvy) + e1z * pvz;
    const v2f inv_det = {1.0f / det.x, 1.0f / det.y};
    const v2f tvx = ro.x - v0x, tvy = ro.y - v0y, tvz = ro.z - v0z;
    u = ((tvx * pvx + tvy * pvy) + tvz * pvz) * inv_det;
    const v2f qvx = tvy * e1z - tvz * e1y, qvy = tvz * e1x - tvx * e1z, qvz = tvx * e1y - tvy * e1x;          // cross(tvec, e1)
    v = ((rd.x * qvx + rd.y * qvy) + rd.z * qvz) * inv_det;
    t = ((e2x * qvx + e2y * qvy) + e2z * qvz) * inv_det;
    const v2f uv = u + v;
    ok_a = !(fabsf(det.x) < 1e-8f) && !(u.x < 0.0f) && !(u.x > 1.0f) && !(v.x < 0.0f) && !(uv.x > 1.0f) && !(t.x < t_min);
    ok_b = !(fabsf(det.y) < 1e-8f) && !(u.y < 0.0f) && !(u.y > 1.0f) && !(v.y < 0.0f) && !(uv.y > 1.0f) && !(t.y < t_min);
}
__device__ __forceinline__ void moller_trumbore_pair(const float4* __restrict__ tp, F3 ro, F3 rd, v2f& t, v2f& u, v2f& v, bool& ok_a, bool& ok_b) {
    moller_trumbore_pair(tp, ro, rd, kTMin, t, u, v, ok_a, ok_b);
}

// One node visit: both child boxes of the pair record (q0, q1, q2, q3) (device_layout.h) against the ray, bbox_hit :285-315 with t_max = `cull`,
// and the child-ordering test :433-453.  Out: whether each child is hit, its slab entry distance, and whether the left child is the nearer one
// (meaningful only when both are hit).  `t_min` as for moller_trumbore_pair.
__device__ __forceinline__ void visit_pair(const float4 q0, const float4 q1, const float4 q2, const float4 q3, F3 ro, F3 rd, F3 rinv, float t_min, float cull,
                                           bool& hl, bool& hr, float& tl, float& tr, bool& left_near) {
    // Both boxes at once: every quantity below is a (left, right) pair in two adjacent registers, so the
    // subtractions / multiplications are packed fp32 ops (v_pk_add_f32 / v_pk_mul_f32: IEEE per component,
    // same results as the scalar forms).  Record layout: q0 = (L.lo.x, R.lo.x, L.hi.x, R.hi.x), q1 = y, q2 = z.
    // (Doing the swap of :305-307 by address -- six 8-byte loads at near/far offsets -- saves the twelve selects
    // but costs three more memory instructions per visit and was 11 % slower: profiles/r01/README.md.)
    const v2f lox = {q0.x, q0.y}, hix = {q0.z, q0.w}, loy = {q1.x, q1.y}, hiy = {q1.z, q1.w}, loz = {q2.x, q2.y}, hiz = {q2.z, q2.w};
    const v2f ax = (lox - ro.x) * rinv.x, bx = (hix - ro.x) * rinv.x;      // bbox_hit :303-304
    const v2f ay = (loy - ro.y) * rinv.y, by = (hiy - ro.y) * rinv.y;
    const v2f az = (loz - ro.z) * rinv.z, bz = (hiz - ro.z) * rinv.z;
    const bool nx = rinv.x < 0.0f, ny = rinv.y < 0.0f, nz = rinv.z < 0.0f;       // the swap of :305-307
    const float t0xl = nx ? bx.x : ax.x, t1xl = nx ? ax.x : bx.x, t0xr = nx ? bx.y : ax.y, t1xr = nx ? ax.y : bx.y;
    const float t0yl = ny ? by.x : ay.x, t1yl = ny ? ay.x : by.x, t0yr = ny ? by.y : ay.y, t1yr = ny ? ay.y : by.y;
    const float t0zl = nz ? bz.x : az.x, t1zl = nz ? az.x : bz.x, t0zr = nz ? bz.y : az.y, t1zr = nz ? az.y : bz.y;
    tl = fmaxf(fmaxf(t_min, t0xl), fmaxf(t0yl, t0zl)); tr = fmaxf(fmaxf(t_min, t0xr), fmaxf(t0yr, t0zr));
    hl = !(fminf(fminf(cull, t1xl), fminf(t1yl, t1zl)) <= tl);
    hr = !(fminf(fminf(cull, t1xr), fminf(t1yr, t1zr)) <= tr);
    // nearer child by box centre along the ray :433-453 (only matters when both are hit).  The reference compares
    //   d = ((c.x - o.x) * dir.x + (c.y - o.y) * dir.y) + (c.z - o.z) * dir.z,   c = 0.5f * (lo + hi)
    // of the two children.  Computed here is 2 d, with the reference's roundings: s = lo + hi is the reference's sum (the x sums come with the record); the product
    // by 0.5f is exact, and fma(-2, o, s) = fl(s - 2 o) = 2 fl(0.5 s - o), because scaling by two commutes with rounding; so do the
    // products and sums that follow.  dL < dR <=> 2 dL < 2 dR, and three packed multiplications per visit are gone.  (The
    // identity needs the reference's intermediates to be zero or normal numbers below 1.7e38: coordinates in metres are.)
    const v2f m2 = {-2.0f, -2.0f}, ox2 = {ro.x, ro.x}, oy2 = {ro.y, ro.y}, oz2 = {ro.z, ro.z};
    const v2f ux = __builtin_elementwise_fma(m2, ox2, (v2f){q3.z, q3.w}), uy = __builtin_elementwise_fma(m2, oy2, loy + hiy), uz = __builtin_elementwise_fma(m2, oz2, loz + hiz);
    const v2f dc = (ux * rd.x + uy * rd.y) + uz * rd.z;
    left_near = dc.x < dc.y;
}

// The walk of bvh_hit_closest :387-473 on the REFERENCE tree (DeviceScene.root_ref), one lane, its stack column `stk` (entry e at stk[e * 64]), for the query
// scene_hit(ray, t_min, closest): near child first by the ordering test, far child pushed, LIFO pop, a leaf's triangles in leaf order, every box tested against
// the shrinking `closest`, equal t accepted (:353).  Closest-hit: on return (closest, slot, u, v) are the accepted triangle of smallest t (slot -1: none).
// ANYHIT: returns at the first accepted triangle.  Used by the G-buffer pass (t_min = 0.001f) and the ray queries (a per-ray t_min).
template <bool ANYHIT>
__device__ __forceinline__ void walk_reference_tree(const DeviceScene& S, uint2* stk, int cap, F3 ro, F3 rd, F3 rinv, float t_min, float& closest, int& slot, float& hu,
                                                    float& hv, uint32_t& status) {
    float t_entry;
    int cur = (S.root_ref != kRefNone && slab(ld3(S.root_lo), ld3(S.root_hi), ro, rinv, t_min, closest, t_entry)) ? S.root_ref : kRefNone;     // :394-410
    int sp = 0;
    while (cur != kRefNone) {
        if (cur == kRefPop) {
            // a postponed child is entered iff its entry distance is still in front of `closest` (bbox_hit of a box known to be hit, :422-424)
            if (sp == 0) { cur = kRefNone; break; }
            --sp;
            const uint2 e = stk[sp * 64];
            if (closest > __uint_as_float(e.y)) cur = (int)e.x;
        } else if (cur >= kRefBias) {
            if (cur - kRefBias >= S.num_pairs) { status |= kFlagBadNodeRef; break; }
            const float4* rec = reinterpret_cast<const float4*>(S.pairs_biased + ((uint32_t)cur << 6));
            const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
            const int ref_l = __float_as_int(q3.x), ref_r = __float_as_int(q3.y);
            bool hl, hr, left_near;
            float tl, tr;
            visit_pair(q0, q1, q2, q3, ro, rd, rinv, t_min, closest, hl, hr, tl, tr, left_near);
            if (hl && hr) {                                                  // far child postponed with its entry distance
                if (sp >= cap) { status |= kFlagStackOverflow; break; }
                stk[sp * 64] = make_uint2((uint32_t)(left_near ? ref_r : ref_l), __float_as_uint(left_near ? tr : tl));
                ++sp;
            }
            const bool take_left = hl && !(hr && !left_near);
            cur = (hl || hr) ? (take_left ? ref_l : ref_r) : kRefPop;
        } else if (cur < 0) {
            int first = leaf_payload(cur), count = leaf_code(cur) + 1;
            if (count == 8) {
                if (first >= S.num_big_leaves) { status |= kFlagBadBigLeaf; break; }
                const int2 bl = S.big_leaves[first]; first = bl.x; count = bl.y;
            }
            if (first < 0 || count < 0 || first + ((count + 1) >> 1) > S.num_tri_pairs) { status |= kFlagBadTriSlot; break; }
            for (int i = 0; i < count; i += 2) {                             // leaf order, A then B of each pair record (:413-420)
                const int pair = first + (i >> 1);
                v2f t, u, v;
                bool ok_a, ok_b;
                moller_trumbore_pair(S.tri_pairs + (size_t)pair * 5, ro, rd, t_min, t, u, v, ok_a, ok_b);
                if (ok_a && !(t.x > closest)) {
                    closest = t.x; slot = pair * 2; hu = u.x; hv = v.x;
                    if (ANYHIT) return;
                }
                if (ok_b && !(t.y > closest)) {                              // an absent B is all zeros: det == 0, never ok
                    closest = t.y; slot = pair * 2 + 1; hu = u.y; hv = v.y;
                    if (ANYHIT) return;
                }
            }
            cur = kRefPop;
        } else {
            status |= kFlagBadNodeRef; break;
        }
    }
}

}  // namespace dsrt
