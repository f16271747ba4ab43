// coverage_kernel.hip -- the sub-pixel coverage pass (include/dsrt.h, COVERAGE: dsrt_render_coverage): n primary rays per pixel through the sub-sample
// positions of a GRID or DIAGONAL pattern, each ray the G-buffer pass's own (gbuffer_kernel.hip) with (jx, jy) in place of (0.5, 0.5); per pixel how many of
// them hit, which, how many of those see the Sun, how many fall into each caller-given triangle range, and every G-buffer channel of one REPRESENTATIVE hit.
//
//   * One lane per sub-sample.  A 64-thread workgroup is one wave and holds P = 64 / n consecutive pixels of the image in linear order: pixel
//     p = workgroup * P + lane / n, sub-sample k = lane % n.  Lanes beyond P * n and lanes of pixels >= W * H are idle.  A wave's pixels may wrap from one
//     row's end to the next row's start; with n = 64 a wave is a pixel and its ballot is the pixel's mask.  The n rays of a pixel are as coherent as rays get.
//   * The walk and the LDS [entry][lane] stack sized by the tree's depth are the G-buffer pass's (walk_common.h); so are the record assembly, the sphere loop, the
//     shadow ray's any-hit tail and the stores of `rep`, which all three query kernels take from hit_record.h (what sharing them did to the device code:
//     profiles/hit_record/device_code_diff.md).
//   * Phase 2: every hit lane that faces the Sun traces its any-hit shadow ray -- all lanes of a pixel group work -- only when a sun output or rep.flags is asked for.
//   * Reduction: the wave's ballot of `hit`, shifted and masked to the pixel group's n bits, is the mask, its popcount the count; the same for the Sun bit and
//     for each class (at most 16 wave-uniform ballots).  The representative: every hit lane forms key << 6 | k and one LDS atomicMin per hit lane on the pixel
//     group's word picks the lane that writes `rep` (an integer minimum: deterministic whatever the order).  Lane k = 0 of a group writes counts, alphas, masks.
//   * No global atomic but the status word; no scratch.
#include "hit_record.h"
#include "launchers.h"

namespace dsrt {

namespace {
constexpr int kCoverageGrid = 0;                                                        // DSRT_COVERAGE_GRID
}

__global__ void __launch_bounds__(64) dsrt_coverage_kernel(const CoverageArgs a) {
    extern __shared__ uint2 cv_stack[];                                      // [entry][lane]
    __shared__ uint32_t rep_word[64];                                        // per pixel group: the smallest key << 6 | k among its hit lanes
    const DeviceScene& S = a.scene;
    const int lane = threadIdx.x;
    const int n = a.n;
    const int grp = lane / n, k = lane - grp * n;
    const size_t n_pixels = (size_t)a.width * (size_t)a.height;
    const size_t p = (size_t)blockIdx.x * (size_t)a.per_wave + (size_t)grp;
    const bool live = grp < a.per_wave && p < n_pixels;
    const int row = live ? (int)(p / (size_t)a.width) : 0, x = live ? (int)(p - (size_t)row * (size_t)a.width) : 0;
    uint2* stk = cv_stack + lane;
    uint32_t status = 0;

    // ---- the sub-sample: its offset in the pixel and its key (include/dsrt.h, COVERAGE) ----
    float jx, jy;
    int key;
    if (a.pattern == kCoverageGrid) {
        const int s = a.samples, j = k / s, i = k - j * s;
        jx = ((float)i + 0.5f) / (float)s;
        jy = ((float)j + 0.5f) / (float)s;
        const int ax = 2 * i + 1 - s, ay = 2 * j + 1 - s;
        key = ax * ax + ay * ay;
    } else {
        jx = jy = ((float)k + 0.5f) / (float)n;
        const int ad = 2 * k + 1 - n;
        key = ad * ad;
    }
    const uint32_t word = (uint32_t)key << 6 | (uint32_t)k;

    // ---- phase 1: the primary ray, make_camera_ray_jittered :941-968; rows top first (kernel row ky = H-1-row) ----
    const int ky = a.height - 1 - row;
    const float u = ((float)x + jx) / (float)(a.width - 1), v = ((float)ky + jy) / (float)(a.height - 1);
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

    // ---- phase 2: the shadow rays of the lanes that hit and face the Sun, any-hit, then the spheres (:809-816) ----
    const bool need_shadow = a.want_sun && hit && cos_t > 0.0f;
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

    // ---- the reduction over a pixel group's n lanes: bits [grp * n, grp * n + n) of a wave ballot ----
    const int shift = grp * n;                                               // <= lane
    const unsigned long long group_bits = n == 64 ? ~0ull : (1ull << n) - 1ull;
    const unsigned long long m_hit = (__builtin_amdgcn_ballot_w64(hit) >> shift) & group_bits;
    const unsigned long long m_sun = (__builtin_amdgcn_ballot_w64(hit && sun_visible) >> shift) & group_bits;
    const int hits = __popcll(m_hit);
    const bool head = live && k == 0;
    if (head) {
        const float fn = (float)n;
        if (a.hits) a.hits[p] = (uint8_t)hits;
        if (a.alpha) a.alpha[p] = (float)hits / fn;
        if (a.mask) a.mask[p] = m_hit;
        const int sun_hits = __popcll(m_sun);
        if (a.sun_hits) a.sun_hits[p] = (uint8_t)sun_hits;
        if (a.sun_alpha) a.sun_alpha[p] = (float)sun_hits / fn;
        if (a.sun_mask) a.sun_mask[p] = m_sun;
    }
    if (a.class_hits) {
        for (int c = 0; c < a.n_classes; ++c) {                              // wave-uniform: one ballot per class
            const int first = a.class_first[c];
            const bool in_c = hit && !h.sphere && h.prim >= first && (uint32_t)(h.prim - first) < (uint32_t)a.class_num[c];
            const unsigned long long m_c = (__builtin_amdgcn_ballot_w64(in_c) >> shift) & group_bits;
            if (head) a.class_hits[p * (size_t)a.n_classes + (size_t)c] = (uint8_t)__popcll(m_c);
        }
    }

    // ---- the representative: the hit lane of smallest key, ties to the smaller k; without a hit, lane k = 0 writes the miss values ----
    if (a.want_rep) {
        rep_word[lane] = 0xFFFFFFFFu;
        __syncthreads();
        if (hit) atomicMin(&rep_word[grp], word);
        __syncthreads();
        const bool writer = hit ? rep_word[grp] == word : (head && hits == 0);
        if (writer) {
            const HitChannels ch = {a.t, a.range, a.depth, a.position, a.normal, a.uv, a.albedo, a.prim_id, a.material_id, a.sun_cos, a.flags};
            store_hit(S, ch, p, h, rd, a.neg_w, cos_t, sun_visible);
        }
    }
    if (status) atomicOr(a.status, status);
}

hipError_t launch_coverage(const CoverageArgs& a, int blocks, hipStream_t stream) {
    hipLaunchKernelGGL(dsrt_coverage_kernel, dim3((unsigned)blocks), dim3(64), (size_t)a.stack_entries * 64 * sizeof(uint2), stream, a);
    return hipGetLastError();
}

}  // namespace dsrt
