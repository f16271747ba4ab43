// bvh_bodies.cpp -- movable rigid bodies on the host: the bodies tree and the CPU statement of a pose update.
//
// NOT the reference's tree and nothing the reference has (it renders one rigid mesh): the contract is include/dsrt.h, MOVABLE RIGID BODIES.
//   * a body is a contiguous range of hs->tris (dsrt_host_scene_begin_body closes the previous range);
//   * dsrt_host_scene_build_bvh_bodies builds one median-split subtree per non-empty body (bvh_median.cpp's builder on the body's range) and joins them by
//     the chain T0 = (body_a, T1), T1 = (body_b, T2), ..., last = (body_y, body_z), all in ONE pre-order node array with global tri_indices;
//   * a rigid motion keeps that topology good, so dsrt_host_scene_set_body_poses only rewrites triangles (from the rest-pose copy, never from the previous pose)
//     and boxes (bottom-up, by the one rule of the header: fminf / fmaxf, canonical zero, pad where a leaf box is flat).
// Every float operation below is a single correctly rounded one in the order the header writes it (the file is compiled with -ffp-contract=off);
// csrc/bodies_kernel.hip does the same arithmetic on the device and tests/_bodies_model.py in numpy.
#include <cmath>
#include <cstring>

#include "host_internal.hpp"

using namespace dsrt;

namespace {

int body_count(const DsrtHostScene& hs) { return (int)hs.body_start.size(); }
int body_first(const DsrtHostScene& hs, int b) { return hs.body_start[b]; }
int body_end(const DsrtHostScene& hs, int b) { return b + 1 < body_count(hs) ? hs.body_start[b + 1] : (int)hs.tris.size(); }

// x' = ((r0*x + r1*y) + r2*z) + t
inline float row(const float* r, float x, float y, float z, float t) { return ((r[0] * x + r[1] * y) + r[2] * z) + t; }
inline void pose_point(const float* p, const float* v, DsrtF3& out) {
    out.x = row(p + 0, v[0], v[1], v[2], p[3]);
    out.y = row(p + 4, v[0], v[1], v[2], p[7]);
    out.z = row(p + 8, v[0], v[1], v[2], p[11]);
}
inline float row_dir(const float* r, float x, float y, float z) { return (r[0] * x + r[1] * y) + r[2] * z; }
inline void pose_dir(const float* p, const float* v, DsrtF3& out) {
    out.x = row_dir(p + 0, v[0], v[1], v[2]);
    out.y = row_dir(p + 4, v[0], v[1], v[2]);
    out.z = row_dir(p + 8, v[0], v[1], v[2]);
}

// The leaf rule: fminf / fmaxf over the leaf's vertices, + 0.0f (a -0 becomes +0), pad where the box is flat.
void leaf_box(const DsrtHostScene& hs, GPUBVHNode& n, float pad) {
    float lo[3], hi[3];
    for (int i = 0; i < n.tri_count; ++i) {
        const GPUTriangle& t = hs.tris[hs.tri_indices[n.tri_offset + i]];
        const float* v = &t.v0.x;                                   // v0, v1, v2: nine floats
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                const float c = v[3 * k + a];
                if (i == 0 && k == 0) lo[a] = hi[a] = c;
                else { lo[a] = fminf(lo[a], c); hi[a] = fmaxf(hi[a], c); }
            }
    }
    for (int a = 0; a < 3; ++a) {
        lo[a] = lo[a] + 0.0f;
        hi[a] = hi[a] + 0.0f;
        if (hi[a] == lo[a]) { lo[a] = lo[a] - pad; hi[a] = hi[a] + pad; }
    }
    n.bbox_min = DsrtF3{lo[0], lo[1], lo[2]};
    n.bbox_max = DsrtF3{hi[0], hi[1], hi[2]};
}

void union_box(const DsrtHostScene& hs, GPUBVHNode& n) {
    const GPUBVHNode& l = hs.nodes[n.left];
    const GPUBVHNode& r = hs.nodes[n.right];
    n.bbox_min = DsrtF3{fminf(l.bbox_min.x, r.bbox_min.x), fminf(l.bbox_min.y, r.bbox_min.y), fminf(l.bbox_min.z, r.bbox_min.z)};
    n.bbox_max = DsrtF3{fmaxf(l.bbox_max.x, r.bbox_max.x), fmaxf(l.bbox_max.y, r.bbox_max.y), fmaxf(l.bbox_max.z, r.bbox_max.z)};
}

// Boxes of one body's subtree, bottom-up: in pre-order a child's number is greater than its parent's.
void refit_body(DsrtHostScene& hs, int b) {
    const int root = hs.body_root[b];
    if (root < 0) return;
    for (int i = root + hs.body_nodes[b] - 1; i >= root; --i) {
        GPUBVHNode& n = hs.nodes[i];
        if (n.tri_count > 0) leaf_box(hs, n, hs.body_pad[b]);
        else union_box(hs, n);
    }
}

void refit_chain(DsrtHostScene& hs) {
    for (size_t i = hs.chain.size(); i-- > 0;) union_box(hs, hs.nodes[hs.chain[i]]);
}

bool is_bodies_tree(const DsrtHostScene* hs) { return hs && hs->bvh_valid && hs->bodies_tree; }

}  // namespace

int dsrt::check_body_poses(int n_bodies, int first_body, int count, const float* poses, const char* fn) {
    const std::string where(fn);
    if (first_body < 1 || count < 0 || first_body > n_bodies || count > n_bodies - first_body) { set_error(where + ": bodies outside 1 .. count - 1"); return DSRT_ERR_INVALID; }
    if (count && !poses) { set_error(where + ": null poses"); return DSRT_ERR_INVALID; }
    for (int i = 0; i < 12 * count; ++i) if (!std::isfinite(poses[i])) { set_error(where + ": a pose entry is not finite"); return DSRT_ERR_INVALID; }
    return DSRT_OK;
}

extern "C" {

int dsrt_host_scene_begin_body(DsrtHostScene* hs) {
    return guarded("dsrt_host_scene_begin_body", [&]() -> int {
    if (!hs) { set_error("dsrt_host_scene_begin_body: null scene"); return DSRT_ERR_INVALID; }
    if (body_count(*hs) >= DSRT_MAX_BODIES) { set_error("dsrt_host_scene_begin_body: a scene has at most DSRT_MAX_BODIES bodies"); return DSRT_ERR_INVALID; }
    hs->body_start.push_back((int)hs->tris.size());
    hs->bodies_tree = false;
    return body_count(*hs) - 1;
    });
}

int dsrt_host_scene_body_count(const DsrtHostScene* hs) { return hs ? body_count(*hs) : 0; }

int dsrt_host_scene_body_range(const DsrtHostScene* hs, int body, int* first_tri, int* num_tris) {
    if (!hs || body < 0 || body >= body_count(*hs)) { set_error("dsrt_host_scene_body_range: no such body"); return DSRT_ERR_INVALID; }
    if (first_tri) *first_tri = body_first(*hs, body);
    if (num_tris) *num_tris = body_end(*hs, body) - body_first(*hs, body);
    return DSRT_OK;
}

int dsrt_host_scene_build_bvh_bodies(DsrtHostScene* hs) {
    return guarded("dsrt_host_scene_build_bvh_bodies", [&]() -> int {
    if (!hs) { set_error("dsrt_host_scene_build_bvh_bodies: null scene"); return DSRT_ERR_INVALID; }
    hs->tri_indices.clear();
    hs->nodes.clear();
    hs->bvh_height = 0;
    hs->bvh_valid = false;
    hs->bodies_tree = false;
    const size_t n = hs->tris.size();
    if (n > (size_t)1 << 28) { set_error("more than 2^28 triangles"); return DSRT_ERR_INVALID; }
    const int B = body_count(*hs);
    hs->body_pad.assign(B, 0.0f);
    hs->body_root.assign(B, -1);
    hs->body_nodes.assign(B, 0);
    hs->chain.clear();
    hs->rest.clear();

    std::vector<TriBox> tri_box(n);
    std::vector<float> centroid(3 * n);
    for (size_t i = 0; i < n; ++i) median_tri_box(hs->tris[i], tri_box[i], &centroid[3 * i]);
    hs->tri_indices.resize(n);
    for (size_t i = 0; i < n; ++i) hs->tri_indices[i] = (int)i;
    hs->nodes.reserve(n * 2 + B);

    std::vector<int> live;                                          // the non-empty bodies, in body order
    for (int b = 0; b < B; ++b) if (body_end(*hs, b) > body_first(*hs, b)) live.push_back(b);
    int height = 0;
    for (size_t j = 0; j < live.size(); ++j) {
        const int b = live[j];
        int level = (int)j + 1;                                     // the chain node above body j is at level j + 1; the last body hangs under the last chain node
        if (j + 1 < live.size()) {
            const int t = (int)hs->nodes.size();
            hs->nodes.emplace_back();
            GPUBVHNode& top = hs->nodes[t];
            std::memset(&top, 0, sizeof top);
            top.left = t + 1;                                       // the body's subtree follows its chain node; .right is set once that subtree is complete
            if (!hs->chain.empty()) hs->nodes[hs->chain.back()].right = t;
            hs->chain.push_back(t);
            if (level > height) height = level;
            level += 1;
        } else if (!hs->chain.empty()) {
            hs->nodes[hs->chain.back()].right = (int)hs->nodes.size();
        }
        const int before = (int)hs->nodes.size();
        const int root = median_subtree(tri_box, centroid, hs->tri_indices, body_first(*hs, b), body_end(*hs, b), level, hs->nodes, height);
        hs->body_root[b] = root;
        hs->body_nodes[b] = (int)hs->nodes.size() - before;
        const GPUBVHNode& r = hs->nodes[root];                       // (still the builder's plain union of the vertices: the unpadded root box)
        const float ex = r.bbox_max.x - r.bbox_min.x, ey = r.bbox_max.y - r.bbox_min.y, ez = r.bbox_max.z - r.bbox_min.z;
        hs->body_pad[b] = flat_box_pad(fmaxf(fmaxf(ex, ey), ez));
    }
    const size_t first_movable = B > 1 ? (size_t)hs->body_start[1] : n;
    hs->rest.resize((n - first_movable) * 18);
    for (size_t i = first_movable; i < n; ++i) std::memcpy(&hs->rest[(i - first_movable) * 18], &hs->tris[i].v0.x, 18 * sizeof(float));

    hs->bvh_height = height;
    hs->bvh_valid = true;
    hs->bodies_tree = true;
    for (int b = 0; b < B; ++b) refit_body(*hs, b);
    refit_chain(*hs);
    if (hs->bvh_height - 1 > 64) {
        set_error("BVH needs a traversal stack deeper than the reference's 64 entries");
        return DSRT_ERR_BVH_DEPTH;
    }
    return DSRT_OK;
    });
}

int dsrt_host_scene_set_body_poses(DsrtHostScene* hs, int first_body, int count, const float* poses) {
    return guarded("dsrt_host_scene_set_body_poses", [&]() -> int {
    if (!hs) { set_error("dsrt_host_scene_set_body_poses: null scene"); return DSRT_ERR_INVALID; }
    if (!is_bodies_tree(hs)) { set_error("dsrt_host_scene_set_body_poses: the scene's tree is not the bodies tree (dsrt_host_scene_build_bvh_bodies)"); return DSRT_ERR_INVALID; }
    const int rc = check_body_poses(body_count(*hs), first_body, count, poses, "dsrt_host_scene_set_body_poses");
    if (rc || !count) return rc;
    const size_t first_movable = (size_t)hs->body_start[1];
    for (int k = 0; k < count; ++k) {
        const int b = first_body + k;
        const float* p = poses + 12 * (size_t)k;
        for (int i = body_first(*hs, b); i < body_end(*hs, b); ++i) {
            const float* r = &hs->rest[((size_t)i - first_movable) * 18];
            GPUTriangle& t = hs->tris[i];
            pose_point(p, r + 0, t.v0); pose_point(p, r + 3, t.v1); pose_point(p, r + 6, t.v2);
            pose_dir(p, r + 9, t.n0); pose_dir(p, r + 12, t.n1); pose_dir(p, r + 15, t.n2);
        }
        refit_body(*hs, b);
    }
    if (count) refit_chain(*hs);
    return DSRT_OK;
    });
}

}  // extern "C"
