// bodies_kernel.hip -- the device half of a pose update (include/dsrt.h, MOVABLE RIGID BODIES; the host half and the contract's CPU statement: host/bvh_bodies.cpp).
//
// Three kinds of launch, enqueued in this order by dsrt_scene_set_body_poses (device_api.hip):
//   transform   one lane per movable PAIR RECORD of the posed bodies: reads the record's two rest-pose triangles (BodiesView::rest_v / rest_n), applies the body's
//               pose, and rewrites the 80-byte record of tri_pairs, the normals of the two 48-byte records of tri_shade (the three ids are kept) and the record's
//               box in pair_box -- all with 16-byte loads and stores;
//   refit       one launch per tree depth, deepest first; one lane per internal node record of a movable subtree.  A leaf child's box is the fold of its pair
//               records' boxes (canonical zero, then the pad where it is flat; a big leaf loops), an internal child's box is the union of the two boxes in that
//               child's own record, which the previous launch finished;
//   chain       one lane walks the chain of top nodes from the last to the first in the same way and leaves the scene's root box in root_box.
// No atomics, no waiting between workgroups: what a launch reads was written by an earlier launch (or, in the chain, earlier by the same lane), so the result is
// a pure function of rest pose and poses.  The arithmetic is the header's, operation for operation (compiled with -ffp-contract=off; fminf / fmaxf are exact).
// Every index read from memory is checked against the array it goes into before it is used.
#include <hip/hip_runtime.h>

#include "launchers.h"

namespace dsrt {

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ float pose_row(const float* r, float x, float y, float z) { return (r[0] * x + r[1] * y) + r[2] * z; }

struct Tri9 { float v[9]; };

__device__ __forceinline__ Tri9 pose_points(const float* p, const Tri9& r) {
    Tri9 o;
    for (int k = 0; k < 3; ++k) {
        const float x = r.v[3 * k], y = r.v[3 * k + 1], z = r.v[3 * k + 2];
        o.v[3 * k + 0] = pose_row(p + 0, x, y, z) + p[3];
        o.v[3 * k + 1] = pose_row(p + 4, x, y, z) + p[7];
        o.v[3 * k + 2] = pose_row(p + 8, x, y, z) + p[11];
    }
    return o;
}
__device__ __forceinline__ Tri9 pose_dirs(const float* p, const Tri9& r) {
    Tri9 o;
    for (int k = 0; k < 3; ++k) {
        const float x = r.v[3 * k], y = r.v[3 * k + 1], z = r.v[3 * k + 2];
        o.v[3 * k + 0] = pose_row(p + 0, x, y, z);
        o.v[3 * k + 1] = pose_row(p + 4, x, y, z);
        o.v[3 * k + 2] = pose_row(p + 8, x, y, z);
    }
    return o;
}
// v0, v1 - v0, v2 - v0: the nine numbers of a triangle in a pair record
__device__ __forceinline__ Tri9 as_record(const Tri9& t) {
    Tri9 q;
    for (int a = 0; a < 3; ++a) { q.v[a] = t.v[a]; q.v[3 + a] = t.v[3 + a] - t.v[a]; q.v[6 + a] = t.v[6 + a] - t.v[a]; }
    return q;
}

__global__ __launch_bounds__(kBlock) void bodies_transform_kernel(BodiesView b, int first, int count) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    const size_t e = (size_t)first + k;
    const float4* rv = b.rest_v + 5 * e;
    const float4* rn = b.rest_n + 5 * e;
    const float4 a0 = rv[0], a1 = rv[1], a2 = rv[2], a3 = rv[3], a4 = rv[4];
    const int pair = __float_as_int(a4.z), tag = __float_as_int(a4.w);
    const int body = tag & 0xFF;
    const bool has_b = (tag >> 8) & 1;
    if ((unsigned)pair >= (unsigned)b.num_tri_pairs || body >= kMaxBodies) return;
    float p[12];
    for (int i = 0; i < 12; ++i) p[i] = b.poses[12 * body + i];

    const Tri9 ra{{a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x}};
    const Tri9 rb{{a2.y, a2.z, a2.w, a3.x, a3.y, a3.z, a3.w, a4.x, a4.y}};
    const Tri9 va = pose_points(p, ra);
    const Tri9 qa = as_record(va);
    Tri9 vb = va, qb{{0, 0, 0, 0, 0, 0, 0, 0, 0}};          // (no B triangle: its half of the record stays zero and the box is A's)
    if (has_b) { vb = pose_points(p, rb); qb = as_record(vb); }

    float4* rec = b.tri_pairs + 5 * (size_t)pair;
    rec[0] = make_float4(qa.v[0], qb.v[0], qa.v[1], qb.v[1]);
    rec[1] = make_float4(qa.v[2], qb.v[2], qa.v[3], qb.v[3]);
    rec[2] = make_float4(qa.v[4], qb.v[4], qa.v[5], qb.v[5]);
    rec[3] = make_float4(qa.v[6], qb.v[6], qa.v[7], qb.v[7]);
    rec[4] = make_float4(qa.v[8], qb.v[8], 0.0f, 0.0f);

    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(fminf(va.v[a], va.v[3 + a]), va.v[6 + a]);
        hi[a] = fmaxf(fmaxf(va.v[a], va.v[3 + a]), va.v[6 + a]);
        lo[a] = fminf(lo[a], fminf(fminf(vb.v[a], vb.v[3 + a]), vb.v[6 + a]));
        hi[a] = fmaxf(hi[a], fmaxf(fmaxf(vb.v[a], vb.v[3 + a]), vb.v[6 + a]));
    }
    b.pair_box[2 * (size_t)pair + 0] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    b.pair_box[2 * (size_t)pair + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);

    const float4 n0 = rn[0], n1 = rn[1], n2 = rn[2], n3 = rn[3], n4 = rn[4];
    const Tri9 na = pose_dirs(p, Tri9{{n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w, n2.x}});
    float4* sh = b.tri_shade + 6 * (size_t)pair;                // two slots of three float4 each
    const float4 ida = sh[2];
    sh[0] = make_float4(na.v[0], na.v[1], na.v[2], na.v[3]);
    sh[1] = make_float4(na.v[4], na.v[5], na.v[6], na.v[7]);
    sh[2] = make_float4(na.v[8], ida.y, ida.z, ida.w);
    if (has_b) {
        const Tri9 nb = pose_dirs(p, Tri9{{n2.y, n2.z, n2.w, n3.x, n3.y, n3.z, n3.w, n4.x, n4.y}});
        const float4 idb = sh[5];
        sh[3] = make_float4(nb.v[0], nb.v[1], nb.v[2], nb.v[3]);
        sh[4] = make_float4(nb.v[4], nb.v[5], nb.v[6], nb.v[7]);
        sh[5] = make_float4(nb.v[8], idb.y, idb.z, idb.w);
    }
}

// The box of the child a node record refers to.
__device__ void child_box(const BodiesView& b, int ref, float pad, float lo[3], float hi[3]) {
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0.0f;
    if (ref_is_leaf(ref)) {
        int first = leaf_payload(ref), count = leaf_code(ref) + 1;
        if (leaf_code(ref) == 7) {
            if ((unsigned)first >= (unsigned)b.num_big_leaves) return;
            const int2 big = b.big_leaves[first];
            first = big.x; count = big.y;
        }
        if (first < 0 || count <= 0) return;
        const int n = (count + 1) >> 1;
        if ((long long)first + n > b.num_tri_pairs) return;
        for (int i = 0; i < n; ++i) {
            const float4 l = b.pair_box[2 * (size_t)(first + i) + 0], h = b.pair_box[2 * (size_t)(first + i) + 1];
            const float pl[3] = {l.x, l.y, l.z}, ph[3] = {h.x, h.y, h.z};
            for (int a = 0; a < 3; ++a) {
                lo[a] = i ? fminf(lo[a], pl[a]) : pl[a];
                hi[a] = i ? fmaxf(hi[a], ph[a]) : ph[a];
            }
        }
        for (int a = 0; a < 3; ++a) {
            lo[a] = lo[a] + 0.0f;
            hi[a] = hi[a] + 0.0f;
            if (hi[a] == lo[a]) { lo[a] = lo[a] - pad; hi[a] = hi[a] + pad; }
        }
    } else if (ref_is_internal(ref)) {
        const int idx = ref - kRefBias;
        if (idx >= b.num_pairs) return;
        const float4* rec = b.pairs + 4 * (size_t)idx;
        const float4 q[3] = {rec[0], rec[1], rec[2]};
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(q[a].x, q[a].y); hi[a] = fmaxf(q[a].z, q[a].w); }
    }
}

__device__ void refit_record(const BodiesView& b, int record, float pad_left, float pad_right) {
    if ((unsigned)record >= (unsigned)b.num_pairs) return;
    float4* rec = b.pairs + 4 * (size_t)record;
    const float4 refs = rec[3];
    float ll[3], lh[3], rl[3], rh[3];
    child_box(b, __float_as_int(refs.x), pad_left, ll, lh);
    child_box(b, __float_as_int(refs.y), pad_right, rl, rh);
    rec[0] = make_float4(ll[0], rl[0], lh[0], rh[0]);
    rec[1] = make_float4(ll[1], rl[1], lh[1], rh[1]);
    rec[2] = make_float4(ll[2], rl[2], lh[2], rh[2]);
    rec[3] = make_float4(refs.x, refs.y, ll[0] + lh[0], rl[0] + rh[0]);
}

__global__ __launch_bounds__(kBlock) void bodies_refit_kernel(BodiesView b, int first, int count) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    const int2 e = b.refit[(size_t)first + k];                  // {node record, body}
    if ((unsigned)e.y >= (unsigned)kMaxBodies) return;
    const float pad = b.pads[e.y];
    refit_record(b, e.x, pad, pad);
}

__global__ void bodies_chain_kernel(BodiesView b) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    for (int i = b.n_chain - 1; i >= 0; --i) {
        const int4 c = b.chain[i];                              // {node record, body of the left child, body of the right child (0 where that is the next top node), -}
        if ((unsigned)c.y >= (unsigned)kMaxBodies || (unsigned)c.z >= (unsigned)kMaxBodies) continue;
        refit_record(b, c.x, b.pads[c.y], b.pads[c.z]);
    }
    float lo[3], hi[3];
    child_box(b, b.root_ref, (unsigned)b.root_body < (unsigned)kMaxBodies ? b.pads[b.root_body] : 0.0f, lo, hi);
    for (int a = 0; a < 3; ++a) { b.root_box[a] = lo[a]; b.root_box[3 + a] = hi[a]; }
}

}  // namespace

hipError_t launch_bodies_transform(const BodiesView& b, int first, int count, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(bodies_transform_kernel, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, b, first, count);
    return hipGetLastError();
}

hipError_t launch_bodies_refit(const BodiesView& b, int first, int count, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(bodies_refit_kernel, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, b, first, count);
    return hipGetLastError();
}

hipError_t launch_bodies_chain(const BodiesView& b, hipStream_t stream) {
    hipLaunchKernelGGL(bodies_chain_kernel, dim3(1), dim3(64), 0, stream, b);
    return hipGetLastError();
}

}  // namespace dsrt
