// render_kernel.hip -- the per-pixel x spp sampling loop as a persistent wave64 kernel for gfx950.
//
// What it computes is src/gpu_render.cu:973-1031 of the reference (render_kernel and everything below it:
// rand01 :77-80, camera ray :941-968, ray_color :715-936, scene_hit :509-551, bvh_hit_closest :387-473,
// bbox_hit :285-315, hit_triangle_index :322-380, hit_sphere :478-504, the scatter functions :603-661, the
// sampling helpers :82-189, tex2D :232-259, tone map + store :1003-1030) -- same fp32 operations in the same
// order, so that with rng_mode 0 the bytes written are the bytes the reference's arithmetic defines.
//
// How it computes it is not the reference's one-thread-per-pixel loop:
//   * Persistent lanes.  A lane owns one pixel at a time (the reference's LCG makes the samples of a pixel one
//     serial stream, :990-999) and pulls the next from a global queue when it finishes, so a wave never idles behind
//     its slowest pixel.  Work items are 8x8-pixel blocks, handed out costliest tile first (scheduling pre-pass,
//     schedule_kernel.hip); with rng_mode 1 (a Philox sub-sequence per sample) the items are slices of a pixel's samples.
//   * A lane is a small state machine (path_machine.h).  The wave alternates between an ADVANCE phase (all lanes
//     that are not walking a ray step their state machine) and a TRAVERSE phase (all lanes with a live ray walk the
//     BVH together, "while-while": node visits together, parked leaves together); phases are left when the lane-slots
//     wasted by the lanes waiting for the other phase exceed what switching costs (ballot + popcount per iteration),
//     which keeps the loops about half full although bounce depths diverge from 1 to 50.
//   * Node visit = ONE 64-byte record with both child boxes, interleaved so the slab arithmetic runs on packed fp32
//     pairs (device_layout.h); the chosen child is not re-tested on entry and a postponed child carries its slab
//     entry distance on the stack, so a pop is a single compare.  Both are bit-identical to the reference's re-tests:
//     see `slab()` in device_math.h and the pop below.
//   * The traversal stack is a short stack in LDS, [entry][lane] so the 64 lanes of a wave hit 64 different banks;
//     entries beyond the LDS part spill to a per-lane strip in global memory (rare, behind a wave-uniform guard).
//     The continuation a lane postpones while its shadow ray is in flight also waits in LDS, not in registers.
//   * The hit record is assembled once per ray from (slot, t, u, v) instead of on every accepted candidate,
//     and shadow rays stop at the first accepted triangle (same boolean as the reference's closest-hit search).
//
//
// This file holds only what is compiled twice: the sampling loop, its four kernel symbols (render, listed, batch, probe) and their launchers.  The pre-pass
// (schedule_kernel.hip), the sample sets' small kernels and resolve (sample_set_kernel.hip) and the hooks (selftest_kernel.hip) are compiled once.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (no fast-math: IEEE div/sqrt are part of the contract).
#include "launchers.h"
#include "path_machine.h"
#include "walk_common.h"

namespace dsrt {
#ifdef DSRT_DEVICE_LIBM
// Second compilation of this file (Makefile: hip_render_kernel_devlibm.o): the same kernels built with the device math library's sinf / cosf / powf (device_math.h)
// and put in a namespace of their own -- DsrtRenderDesc.math_mode 1.
namespace devlibm {
#endif
// Register budget: 4 waves per SIMD (= 4 blocks per CU, which is also what the blocks' 31 KB of LDS allow).
#ifndef DSRT_WAVES_ATTR
#define DSRT_WAVES_ATTR __attribute__((amdgpu_waves_per_eu(4)))
#endif

// The accepts of one pair record (moller_trumbore_pair, walk_common.h, evaluates both triangles in full) in the reference's order (:353, :371-379): A, then B against the `closest` A may have just lowered.
// `slot_a` = slot of triangle A.  Returns true when the walk is over (an any-hit shadow ray found its blocker).
template <bool COUNT, bool ANYHIT>
__device__ __forceinline__ bool apply_pair(Lane& ln, uint32_t* c, int slot_a, v2f t, v2f u, v2f v, bool ok_a, bool ok_b, bool has_b) {
    bool stop = false;
    if (COUNT) c[C_TRI_TESTS]++;
    if (ok_a && !(t.x > ln.closest)) {
        // (certified second tree, path_machine.h) an equality accept over an earlier hit is a TIE: the reference's answer would depend on its own order
        ln.aux = (t.x == ln.closest && ln.hit_slot >= 0) ? (ln.aux | kTie) : (ln.aux & ~kTie);
        ln.closest = t.x; ln.cull = t.x * ln.relax; ln.hit_slot = slot_a; ln.hit_u = u.x; ln.hit_v = v.x;
        if (COUNT) c[C_HIT_UPDATES]++;
        stop = ANYHIT && ln.state == ST_TRAV_SHADOW;
    }
    if (COUNT && has_b && !stop) c[C_TRI_TESTS]++;
    if (!stop && ok_b && !(t.y > ln.closest)) {          // an absent B is all zeros: det == 0, never ok
        ln.aux = (t.y == ln.closest && ln.hit_slot >= 0) ? (ln.aux | kTie) : (ln.aux & ~kTie);
        ln.closest = t.y; ln.cull = t.y * ln.relax; ln.hit_slot = slot_a + 1; ln.hit_u = u.y; ln.hit_v = v.y;
        if (COUNT) c[C_HIT_UPDATES]++;
        stop = ANYHIT && ln.state == ST_TRAV_SHADOW;
    }
    return stop;
}

// Node-loop iterations per look at the loop's votes (1: +1.4 % time, 3: no better than 2; profiles/r03/ab_node_loop_unroll.jsonl).
constexpr int kNodeUnroll = 2;

template <int K, bool COUNT, bool CHECKED, bool ANYHIT, int RNGMODE, bool PROBE, bool BATCH = false, bool LEAN = false, bool SETS = false, bool MOMENTS = false, bool LISTED = false>
__device__ __forceinline__ void render_body(const RenderArgs& args) {
    const DeviceScene& S = args.scene;
    __shared__ uint2 lds_stack[kWavesPerBlock][K + 1][64];       // entry K is a dump slot, see the node visit

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint32_t glane = blockIdx.x * blockDim.x + threadIdx.x;

    __shared__ float lds_pend[kPendWords][kPendStride];
    LaneOf<MOMENTS> ln;
    ln.pend = &lds_pend[0][threadIdx.x];
    ln.aux = (uint32_t)lane;
    int& state = ln.state; int& cur = ln.cur; int& sp = ln.sp;
    uint32_t& steps = ln.steps;
    F3& ro = ln.ro; F3& rd = ln.rd; F3& rinv = ln.rinv;
    uint32_t c[kNumCounters];
#pragma unroll
    for (int i = 0; i < kNumCounters; ++i) c[i] = 0;
    uint32_t flags = 0;
    const unsigned long long t_enter = COUNT ? wall_clock64() : 0ull;
    if (lane == 0) mark_time<COUNT>(args, C_T_FIRST);

    for (;;) {
        // =====================================================================================
        // ADVANCE phase
        // =====================================================================================
        for (int budget = 0; budget < args.advance_budget; ++budget) {
            // lanes whose delegated shadow ray (path_machine.h) has not answered yet step aside; those whose answer came are back
            if (wave_any((ln.aux & kAwait) != 0u)) {
                if (ln.aux & kAwait) {
                    lane_handoff_acquire();
                    const bool answered = ln.pend[12 * kPendStride] != 0.0f;
                    if (state >= kParked) { if (answered) state -= kParked; }
                    else if (state < ST_TRAV_CLOSEST && !answered) state += kParked;
                }
            }
            if (!wave_any(state < ST_TRAV_CLOSEST)) break;
            if (COUNT) { c[C_ADV_SLOTS]++; if (state < ST_TRAV_CLOSEST) c[C_ADV_ACTIVE]++; }
            // idle lanes go through the step too: that is where they pick up shadow rays
            if (state < ST_TRAV_CLOSEST || state == ST_DONE) {
                // The pass reads its launch constants (camera, sun, sizes, scene pointers) from the kernel-argument segment WHERE IT USES THEM -- scalar loads through the
                // constant cache -- instead of keeping ~60 scalar registers alive across the whole kernel for them: the pointer goes through an empty asm, so the
                // compiler cannot hoist the loads out of the loop and then spill their results to vector lanes (105 spilled scalars, 170 v_readlane / v_writelane in this
                // pass, before; none now, and 112 VGPRs instead of 128.  Time: unchanged within the noise, profiles/r04/ab_kernarg_reload_*.jsonl).
                typedef const RenderArgs __attribute__((address_space(4)))* KernargPtr;
                KernargPtr kp = (KernargPtr)__builtin_amdgcn_kernarg_segment_ptr();
                asm volatile("" : "+s"(kp));
                advance_step<COUNT, CHECKED, ANYHIT, RNGMODE, PROBE, BATCH, LEAN, SETS, MOMENTS, LISTED>(ln, *(const RenderArgs*)kp, c, flags);
            }
        }

        if (wave_all(state == ST_DONE)) break;

        if constexpr (!PROBE && RNGMODE == 0) {
            // Waves that hold a pixel of a heavy tile ask the SIMD's arbiter for priority over waves that only hold background pixels
            // (levels: device_api.hip).  Scheduling only.
            if (args.hot) {
                if (wave_any((ln.aux & kHot) != 0u)) __builtin_amdgcn_s_setprio(3);
                else __builtin_amdgcn_s_setprio(0);
            }
        }

        // =====================================================================================
        // TRAVERSE phase ("while-while"), written flat: per wave iteration every lane that is descending performs at most
        // one POP ATTEMPT and one NODE VISIT, both as straight predicated code (no inner loops, no nested branches); lanes
        // that reached a leaf PARK there until enough lanes are parked, then all parked leaves are intersected together,
        // one triangle index at a time.  Each lane still performs exactly the reference's sequence of box tests,
        // triangle tests and pops -- only WHEN a lane runs changes, never what it does.
        //   cur >= kRefBias: internal node to visit          cur == kRefPop: take the next postponed child
        //   cur <  0            : parked at a leaf          cur == kRefNone: no ray
        // =====================================================================================
        // Leaving a phase is decided by accumulated waste, in lane-slots: every wave iteration spent here costs the lanes
        // that are waiting for the OTHER phase one slot each; switching costs the lanes that are busy HERE one pass of the
        // other phase.  Switch when the first exceeds the second (the ratios are the relative lengths of the phases' code).
        // Invariant used for the votes below: a lane that is not walking a ray has cur == kRefNone, so "walking" and its
        // refinements are single compares on `cur` (a vote on one compare is the compare's own mask, no extra VALU work).
        for (int wait_waste = 0;;) {
            const int n_walk = __popcll(wave_ballot(cur != kRefNone));
            if (n_walk == 0) break;
            const int n_wait = __popcll(wave_ballot(state < ST_TRAV_CLOSEST));
            if (wait_waste * 10 >= n_walk * args.min_walk_iters) break;
            int leaf_waste = 0;

            // ---------------- phase I: pops and internal nodes ----------------
            for (;;) {
                const bool descending = cur > kRefNone;                                              // kRefPop or an internal node
                const int n_desc = __popcll(wave_ballot(descending));
                const int n_leaf = __popcll(wave_ballot(cur < 0));
                if (n_desc == 0 || leaf_waste * 10 >= n_desc * args.leaf_ratio4) break;
                // Two iterations per look at the votes: the loop's own bookkeeping (two compares, seven scalar instructions, two branches) is paid every other time.
                leaf_waste += kNodeUnroll * n_leaf;
                wait_waste += kNodeUnroll * n_wait;
#pragma unroll
                for (int rep = 0; rep < kNodeUnroll; ++rep) {           // (body not re-indented: it is the iteration described above)
                // (checked build) a reference in 0 .. kRefNone - 1 belongs to no class: such a lane would be counted as walking for ever.  Library-built records never hold one;
                // a corrupted record or stack word might.
                if (CHECKED && cur >= 0 && cur < kRefNone) { flags |= kFlagBadNodeRef; cur = kRefNone; }
                if (COUNT) { c[C_NODE_SLOTS]++; if (cur < 0) c[C_IDLE_AT_LEAF]++; if (state < ST_TRAV_CLOSEST || (cur == kRefNone && state <= ST_TRAV_SHADOW)) c[C_IDLE_WAITING]++; if (state == ST_DONE) c[C_IDLE_DONE]++; }

                // pop attempt: a postponed child is entered iff its entry distance is still in front of `closest`, which is
                // bbox_hit(node, ray, t_min, closest) for a box already known to be hit (src/gpu_render.cu:422-424, 462-468)
                {
                    const bool popping = cur == kRefPop;
                    const bool finished = popping && sp == 0;
                    // a ray that has emptied its stack: its state leaves ST_TRAV_* when the node loop is left (below), not here, every iteration
                    if (finished) cur = kRefNone;
                    if (popping != finished) {                 // popping with something on the stack (one compare of sp, not two)
                        --sp;
                        uint2 e = lds_stack[wave][sp < K ? sp : K][lane];
                        if (wave_any(sp >= K)) {               // wave-uniform guard: keeps the common path a plain ds_read_b64 (without it: +3 %)
                            if (sp >= K) e = args.spill[(size_t)(sp - K) * args.spill_stride + glane];
                        }
                        if (ln.cull > __uint_as_float(e.y)) cur = (int)e.x;                // (cull == closest on the reference tree: the reference's own test)
                    }
                }

                // node visit: both child boxes from one 64-byte record
                if (cur > kRefPop) {
                    if (CHECKED && (cur - kRefBias >= S.num_pairs || ++steps > kStepCap)) {
                        flags |= cur - kRefBias >= S.num_pairs ? kFlagBadNodeRef : kFlagStepCap;
                        cur = kRefNone; state -= (ST_TRAV_CLOSEST - ST_SHADE);
                    } else {
                        const float4* rec = reinterpret_cast<const float4*>(S.pairs_biased + ((uint32_t)cur << 6));     // 32-bit offset from a scalar base (num_pairs < 2^26 - 64, checked at upload)
                        const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
                        const int ref_l = __float_as_int(q3.x), ref_r = __float_as_int(q3.y);
                        if (COUNT) { c[C_NODES_ENTERED]++; c[C_INTERNAL_ENTERED]++; c[C_BOX_FETCHES] += 2; const int dpt = S.pair_depth[cur - kRefBias]; if (dpt < 6) c[C_VISITS_LT6]++; if (dpt < 9) c[C_VISITS_LT9]++; if (dpt < 12) c[C_VISITS_LT12]++; }
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
                        const float tl = fmaxf(fmaxf(kTMin, t0xl), fmaxf(t0yl, t0zl)), tr = fmaxf(fmaxf(kTMin, t0xr), fmaxf(t0yr, t0zr));
                        const bool hl = !(fminf(fminf(ln.cull, t1xl), fminf(t1yl, t1zl)) <= tl);
                        const bool hr = !(fminf(fminf(ln.cull, t1xr), fminf(t1yr, t1zr)) <= tr);
                        // nearer child by box centre along the ray :433-453 (only matters when both are hit).  The reference compares
                        //   d = ((c.x - o.x) * dir.x + (c.y - o.y) * dir.y) + (c.z - o.z) * dir.z,   c = 0.5f * (lo + hi)
                        // of the two children.  Computed here is 2 d, with the reference's roundings: s = lo + hi is the reference's sum (the x sums come with the record); the product
                        // by 0.5f is exact, and fma(-2, o, s) = fl(s - 2 o) = 2 fl(0.5 s - o), because scaling by two commutes with rounding; so do the
                        // products and sums that follow.  dL < dR <=> 2 dL < 2 dR, and three packed multiplications per visit are gone.  (The
                        // identity needs the reference's intermediates to be zero or normal numbers below 1.7e38: coordinates in metres are.)
                        const v2f m2 = {-2.0f, -2.0f}, ox2 = {ro.x, ro.x}, oy2 = {ro.y, ro.y}, oz2 = {ro.z, ro.z};
                        const v2f ux = __builtin_elementwise_fma(m2, ox2, (v2f){q3.z, q3.w}), uy = __builtin_elementwise_fma(m2, oy2, loy + hiy), uz = __builtin_elementwise_fma(m2, oz2, loz + hiz);
                        const v2f dc = (ux * rd.x + uy * rd.y) + uz * rd.z;
                        const bool left_near = dc.x < dc.y;
                        const bool both = hl && hr;
                        // the far child goes to stack[sp]; written unconditionally (slot sp is above the top, slot K is a dump
                        // slot for sp >= K), the stack only grows when both children were hit
                        const uint2 far = make_uint2((uint32_t)(left_near ? ref_r : ref_l), __float_as_uint(left_near ? tr : tl));
                        lds_stack[wave][sp < K ? sp : K][lane] = far;
                        if (both && sp >= K) {                             // the rare spill store (a vote shared by the two sites, at the top of the iteration, was 1 % slower)
                            if (sp - K < args.spill_entries) {
                                args.spill[(size_t)(sp - K) * args.spill_stride + glane] = far;
                                if (COUNT) c[C_STACK_SPILLS]++;
                            } else flags |= kFlagStackOverflow;
                        }
                        sp += both ? 1 : 0;
                        if (COUNT && (uint32_t)sp > c[C_MAX_STACK]) c[C_MAX_STACK] = (uint32_t)sp;
                        // next node, without branches: the left child if both were hit and it is the nearer one, or if it alone was hit
                        const bool take_left = hl && !(hr && !left_near);            // (written as mask logic: a select between two predicates compiles to five VALU instructions)
                        const int child = take_left ? ref_l : ref_r;
                        cur = (hl || hr) ? child : kRefPop;
                    }
                }
                }                                                       // rep
            }

            if (CHECKED && cur >= 0 && cur < kRefNone) { flags |= kFlagBadNodeRef; cur = kRefNone; }       // (a bad reference taken in the loop's last iteration)
            // rays that emptied their stack in the node loop: TRAV_CLOSEST -> SHADE, TRAV_SHADOW -> SHADOW_DONE (a lane in ST_TRAV_* without a node has just ended)
            if (cur == kRefNone && state >= ST_TRAV_CLOSEST && state <= ST_TRAV_SHADOW) state -= (ST_TRAV_CLOSEST - ST_SHADE);

            // ---------------- phase L: every lane parked at a leaf intersects it, triangle by triangle :413-420 ----------------
            const bool at_leaf = cur < 0;
            const unsigned long long leaf_mask = wave_ballot(at_leaf);
            if (leaf_mask != 0ull) {
                wait_waste += n_wait;
                int first = 0, count = 0;
                if (at_leaf) {
                    first = leaf_payload(cur);
                    count = leaf_code(cur) + 1;
                    if (count == 8) {
                        if (CHECKED && first >= S.num_big_leaves) { flags |= kFlagBadBigLeaf; first = 0; count = 0; }
                        else { const int2 bl = S.big_leaves[first]; first = bl.x; count = bl.y; }
                    }
                    if (CHECKED && (first < 0 || first + ((count + 1) >> 1) > S.num_tri_pairs || ++steps > kStepCap)) { flags |= kFlagBadTriSlot; count = 0; }
                    if (COUNT) c[C_NODES_ENTERED]++;
                    cur = kRefPop;
                }
                // Two triangles (one pair record) per step.  Every quantity is an (A, B) pair in adjacent registers; both
                // tests are evaluated in full against nothing but the ray, then APPLIED in the reference's order: A first, and
                // B against the `closest` A may have just lowered -- the reference's sequence of accepts, bit for bit.
                //
                // Second records are DEALT to the lanes that are not at a leaf.  The median-split builder stops at four triangles, so
                // nearly every leaf of a large mesh is two pair records, while at most a third of the wave is parked when this pass
                // runs: the loop used to run twice at a quarter of its lanes.  Evaluating a record needs the ray and the record, not
                // `closest`; only the accepts are ordered.  So the r-th lane that is not at a leaf evaluates record 1 of the r-th
                // parked lane that has one (the ray comes over by ds_bpermute; its own registers are untouched), hands (t, u, v, ok)
                // of both triangles back the same way, and the owner applies A, B of record 0 and then A, B of record 1 -- the
                // reference's order.  Taken only when EVERY second record finds a lane (otherwise the second trip is paid anyway).
                // Leaves of more than four triangles (coincident centroids) finish in the plain loop below.
                int done = 0;                                              // triangles of this lane's leaf dealt with so far
                if (args.deal_leaves) {
                    const bool want = count > 2;
                    const unsigned long long want_mask = wave_ballot(want);
                    const int n_want = __popcll(want_mask);
                    if (n_want > 0 && n_want <= 64 - __popcll(leaf_mask)) {
                        const uint32_t rank_w = __builtin_amdgcn_mbcnt_hi((uint32_t)(want_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)want_mask, 0u));
                        const uint32_t rank_i = __builtin_amdgcn_mbcnt_hi((uint32_t)(~leaf_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)~leaf_mask, 0u));
                        float* const table = ln.pend + 13 * kPendStride - lane;          // the wave's 64-entry table (free outside advance_step)
                        const bool helping = !at_leaf && rank_i < (uint32_t)n_want;
                        if (want) table[rank_w] = __int_as_float(lane);
                        lane_handoff_release();
                        int src = lane;                                      // whose ray this lane evaluates: its own, or its owner's
                        if (helping) { lane_handoff_acquire(); src = __float_as_int(table[rank_i]); table[rank_i] = __int_as_float(lane); }
                        lane_handoff_release();
                        const int src4 = src << 2;
                        const F3 lro = mk(__int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(ro.x))), __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(ro.y))),
                                          __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(ro.z))));
                        const F3 lrd = mk(__int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(rd.x))), __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(rd.y))),
                                          __int_as_float(__builtin_amdgcn_ds_bpermute(src4, __float_as_int(rd.z))));
                        const int lpair = __builtin_amdgcn_ds_bpermute(src4, first) + (helping ? 1 : 0);
                        v2f t, u, v;                                         // meaningful only where `ok` says so (unset elsewhere: six moves per pass)
                        int ok = 0;                                          // bit 0: A passed every test but the one against `closest`, bit 1: B
                        if (COUNT) c[C_TRI_SLOTS] += 2;
                        if (count > 0 || helping) {                          // (count is 0 in the lanes that are not at a leaf: two plain compares, not a select between predicates)
                            bool ok_a, ok_b;
                            moller_trumbore_pair(S.tri_pairs + (size_t)lpair * 5, lro, lrd, t, u, v, ok_a, ok_b);
                            ok = (ok_a ? 1 : 0) | (ok_b ? 2 : 0);
                        }
                        // the owner fetches its helper's results (a lane without one reads its own and ignores them)
                        int from = lane;
                        if (want) { lane_handoff_acquire(); from = __float_as_int(table[rank_w]); }
                        const int from4 = from << 2;
                        const v2f t2 = {__int_as_float(__builtin_amdgcn_ds_bpermute(from4, __float_as_int(t.x))), __int_as_float(__builtin_amdgcn_ds_bpermute(from4, __float_as_int(t.y)))};
                        const v2f u2 = {__int_as_float(__builtin_amdgcn_ds_bpermute(from4, __float_as_int(u.x))), __int_as_float(__builtin_amdgcn_ds_bpermute(from4, __float_as_int(u.y)))};
                        const v2f v2 = {__int_as_float(__builtin_amdgcn_ds_bpermute(from4, __float_as_int(v.x))), __int_as_float(__builtin_amdgcn_ds_bpermute(from4, __float_as_int(v.y)))};
                        const int ok2 = __builtin_amdgcn_ds_bpermute(from4, ok);
                        if (at_leaf && count > 0) {
                            bool stop = apply_pair<COUNT, ANYHIT>(ln, c, first * 2, t, u, v, (ok & 1) != 0, (ok & 2) != 0, count > 1);
                            if (!stop && want) stop = apply_pair<COUNT, ANYHIT>(ln, c, first * 2 + 2, t2, u2, v2, (ok2 & 1) != 0, (ok2 & 2) != 0, count > 3);
                            done = want ? 4 : 2;
                            if (stop) { count = 0; cur = kRefNone; state = ST_SHADOW_DONE; }
                        }
                    }
                }
                for (int i = done; wave_any(i < count); i += 2) {
                    if (COUNT) c[C_TRI_SLOTS] += 2;
                    if (i < count) {
                        const int pair = first + (i >> 1);
                        v2f t, u, v;
                        bool ok_a, ok_b;
                        moller_trumbore_pair(S.tri_pairs + (size_t)pair * 5, ro, rd, t, u, v, ok_a, ok_b);
                        if (apply_pair<COUNT, ANYHIT>(ln, c, pair * 2, t, u, v, ok_a, ok_b, i + 1 < count)) { count = 0; cur = kRefNone; state = ST_SHADOW_DONE; }
                    }
                }
            }
        }
    }

    if (COUNT && lane == 0) c[C_WAVE_TICKS] = (uint32_t)(wall_clock64() - t_enter);
    if (lane == 0) mark_time<COUNT>(args, C_T_LAST);
    flush_counters<COUNT>(args, c);
    if (flags) atomicOr(args.flags, flags);
}

// LEAN (path_machine.h): the instantiation for scenes of Lambertian triangles only, chosen by the host from what upload found in the scene.  Production builds only:
// the counting and checked builds are the general code.  SETS, MOMENTS (path_machine.h): the rng_mode 1 launches of dsrt_render_accumulate, built beside
// dsrt_render's own.
template <int K, bool COUNT, bool CHECKED, bool ANYHIT, int RNGMODE, bool LEAN = false, bool SETS = false, bool MOMENTS = false>
__global__ void __launch_bounds__(64 * kWavesPerBlock) DSRT_WAVES_ATTR dsrt_render_kernel(const RenderArgs args) {
    static_assert(!SETS || RNGMODE == 1, "sample sets are rng_mode 1's");
    static_assert(!MOMENTS || SETS, "second moments are summed by accumulate launches only");
    render_body<K, COUNT, CHECKED, ANYHIT, RNGMODE, false, false, LEAN, SETS, MOMENTS>(args);
}

// Masked accumulate launch (dsrt_render_accumulate_masked): the SETS kernel of rng_mode 1 with its work items fetched from the lists of active pixels
// (path_machine.h, LISTED).  Production (LEAN or general) and checked builds only.  A kernel symbol of its own: dsrt_render_kernel's instantiations keep their names.
template <bool CHECKED, bool LEAN, bool MOMENTS>
__global__ void __launch_bounds__(64 * kWavesPerBlock) DSRT_WAVES_ATTR dsrt_render_listed_kernel(const RenderArgs args) {
    static_assert(!(CHECKED && LEAN), "the checked build is the general code");
    render_body<8, false, CHECKED, true, 1, false, false, LEAN, true, MOMENTS, true>(args);
}

// Batch launch: many frames of one scene as one pool of work (path_machine.h, ST_FETCH).
template <int RNGMODE, bool LEAN = false>
__global__ void __launch_bounds__(64 * kWavesPerBlock) DSRT_WAVES_ATTR dsrt_render_batch_kernel(const RenderArgs args) {
    render_body<8, false, false, true, RNGMODE, false, true, LEAN>(args);
}

// The probe launch of the pre-pass: the same body at a couple of samples per pixel, adding the rays every pixel needed to its
// tile's entry of args.tile_work.  Its own kernel symbol, so that profiles keep it apart from the frame's launch.
template <bool LEAN>
__global__ void __launch_bounds__(64 * kWavesPerBlock) DSRT_WAVES_ATTR dsrt_probe_kernel(const RenderArgs args) {
    render_body<8, false, false, true, 0, true, false, LEAN>(args);
}

// ---- launchers (launchers.h: they go out as this compilation's table) -----
template <int K, int RNGMODE, bool SETS = false, bool MOMENTS = false>
static hipError_t launch_k(const RenderArgs& a, int blocks, bool count, bool checked, bool anyhit, bool lean, hipStream_t stream) {
    const dim3 grid(blocks), block(64 * kWavesPerBlock);
    if (!count && !checked && lean) {
        hipLaunchKernelGGL((dsrt_render_kernel<K, false, false, true, RNGMODE, true, SETS, MOMENTS>), grid, block, 0, stream, a);
    } else if (count) {
        if (anyhit) hipLaunchKernelGGL((dsrt_render_kernel<K, true, true, true, RNGMODE, false, SETS, MOMENTS>), grid, block, 0, stream, a);
        else        hipLaunchKernelGGL((dsrt_render_kernel<K, true, true, false, RNGMODE, false, SETS, MOMENTS>), grid, block, 0, stream, a);
    } else if (checked) {
        hipLaunchKernelGGL((dsrt_render_kernel<K, false, true, true, RNGMODE, false, SETS, MOMENTS>), grid, block, 0, stream, a);
    } else {
        hipLaunchKernelGGL((dsrt_render_kernel<K, false, false, true, RNGMODE, false, SETS, MOMENTS>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

static hipError_t launch_render_batch(const RenderArgs& a, int rng_mode, int blocks, bool lean, hipStream_t stream) {
    const dim3 grid(blocks), block(64 * kWavesPerBlock);
    if (rng_mode == 0) { if (lean) hipLaunchKernelGGL((dsrt_render_batch_kernel<0, true>), grid, block, 0, stream, a); else hipLaunchKernelGGL((dsrt_render_batch_kernel<0, false>), grid, block, 0, stream, a); }
    else if (rng_mode == 1) { if (lean) hipLaunchKernelGGL((dsrt_render_batch_kernel<1, true>), grid, block, 0, stream, a); else hipLaunchKernelGGL((dsrt_render_batch_kernel<1, false>), grid, block, 0, stream, a); }
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

static hipError_t launch_probe(const RenderArgs& a, int blocks, bool lean, hipStream_t stream) {
    if (lean) hipLaunchKernelGGL(dsrt_probe_kernel<true>, dim3(blocks), dim3(64 * kWavesPerBlock), 0, stream, a);
    else hipLaunchKernelGGL(dsrt_probe_kernel<false>, dim3(blocks), dim3(64 * kWavesPerBlock), 0, stream, a);
    return hipGetLastError();
}

template <bool MOMENTS>
static hipError_t launch_listed(const RenderArgs& a, int blocks, bool checked, bool lean, hipStream_t stream) {
    const dim3 grid(blocks), block(64 * kWavesPerBlock);
    if (checked) hipLaunchKernelGGL((dsrt_render_listed_kernel<true, false, MOMENTS>), grid, block, 0, stream, a);
    else if (lean) hipLaunchKernelGGL((dsrt_render_listed_kernel<false, true, MOMENTS>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((dsrt_render_listed_kernel<false, false, MOMENTS>), grid, block, 0, stream, a);
    return hipGetLastError();
}

// sets: the SETS instantiations (rng_mode 1, dsrt_render_accumulate); moments: with MOMENTS as well (a.accum_sq is set); listed: the masked form of a SETS launch
// (K = 8 is the only short-stack size built)
static hipError_t launch_render(const RenderArgs& a, const RenderVariant& v, int blocks, hipStream_t stream) {
    if (v.listed) {
        if (v.rng_mode != 1 || !v.sets || v.count || !v.anyhit) return hipErrorInvalidValue;
        return v.moments ? launch_listed<true>(a, blocks, v.checked, v.lean, stream) : launch_listed<false>(a, blocks, v.checked, v.lean, stream);
    }
    if (v.rng_mode == 0 && !v.sets && !v.moments) return launch_k<8, 0>(a, blocks, v.count, v.checked, v.anyhit, v.lean, stream);
    if (v.rng_mode == 1 && !v.sets && !v.moments) return launch_k<8, 1>(a, blocks, v.count, v.checked, v.anyhit, v.lean, stream);
    if (v.rng_mode == 1 && v.sets && !v.moments) return launch_k<8, 1, true>(a, blocks, v.count, v.checked, v.anyhit, v.lean, stream);
    if (v.rng_mode == 1 && v.sets && v.moments) return launch_k<8, 1, true, true>(a, blocks, v.count, v.checked, v.anyhit, v.lean, stream);
    return hipErrorInvalidValue;
}

const RenderLaunchers& compiled_render_launchers() {
    static const RenderLaunchers table = {launch_render, launch_render_batch, launch_probe};
    return table;
}

#ifdef DSRT_DEVICE_LIBM
}  // namespace devlibm
#endif
}  // namespace dsrt
